// tests/compat_runtime: a working stand-in for the small part of OpenCV 3.2's cv::Mat that compat/ runs on (see README.md in
// this directory).  Only CV_8U and CV_32F single-channel matrices exist.  Storage is reference counted and rowRange / colRange /
// row / col are views that share it and its row step, as in OpenCV; clone() and t() copy into a fresh continuous buffer.
// oracle/ref/matcher/ compiles the reference's src/ORBmatcher.cc and src/MapPoint.cc against this same file.
//
// Arithmetic (CV_32F only; every result is a fresh matrix, and MatExpr is simply Mat):
//   a + b, a - b, -a        element-wise in float
//   s * a, a * s, a / s     element-wise, computed in double from the float element and the double scalar, rounded once
//   a * b                   matrix product: C(i,j) = sum over k = 0, 1, ... of A(i,k) * B(k,j), accumulated in double in that
//                           order, rounded once to float (OpenCV's gemm also widens float products to a double accumulator)
//   a.dot(b), norm(a)       sums over the elements in row-major order, accumulated in double; norm returns sqrt of that sum
// The compat tests feed exact (dyadic) values, for which every order of summation gives the same result.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#define CV_8U 0
#define CV_32F 5
#define CV_8UC1 0
#define CV_Assert(expr) do { if (!(expr)) throw std::runtime_error("CV_Assert failed: " #expr); } while (0)

namespace cv {

struct Point2f {
    float x, y;
    Point2f() : x(0.f), y(0.f) {}
    Point2f(float x_, float y_) : x(x_), y(y_) {}
};

template <typename T> struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T x_, T y_) : x(x_), y(y_) {}
};
typedef Point_<int> Point2i;
typedef Point2i Point;

// the 28-byte POD of OpenCV 3.2 (pt, size, angle, response, octave, class_id); compat/ static_asserts the size
struct KeyPoint {
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
};

class Mat {
public:
    int rows, cols;
    unsigned char *data;
    size_t step;

    Mat() : rows(0), cols(0), data(NULL), step(0), type_(CV_8U) {}
    Mat(int r, int c, int type) : rows(0), cols(0), data(NULL), step(0), type_(CV_8U) { create(r, c, type); }
    // wraps caller-owned memory (no reference count), as OpenCV's user-data constructor does
    Mat(int r, int c, int type, void *ext) : rows(r), cols(c), data((unsigned char *)ext), step((size_t)c * ElemSize(type)), type_(type) {}

    int type() const { return type_; }
    size_t elemSize() const { return ElemSize(type_); }
    bool empty() const { return data == NULL || rows == 0 || cols == 0; }
    size_t total() const { return (size_t)rows * cols; }
    bool isContinuous() const { return rows <= 1 || step == (size_t)cols * elemSize(); }

    void create(int r, int c, int type) {
        if (data && rows == r && cols == c && type_ == type) return;   // OpenCV keeps the buffer when nothing changes
        CV_Assert(r >= 0 && c >= 0 && (type == CV_8U || type == CV_32F));
        type_ = type; rows = r; cols = c; step = (size_t)c * ElemSize(type);
        buf_ = std::make_shared<std::vector<unsigned char> >(std::max<size_t>((size_t)r * step, 1), 0);
        data = buf_->data();
    }
    void release() { buf_.reset(); data = NULL; rows = cols = 0; step = 0; }

    Mat clone() const {
        Mat m(rows, cols, type_);
        for (int r = 0; r < rows; ++r) std::memcpy(m.ptr(r), ptr(r), (size_t)cols * elemSize());
        return m;
    }
    // copies into dst's storage; a temporary dst is a header (usually _OutputArray::getMat() after create) of the same shape
    // and type; a named dst is (re)allocated first when its shape or type differs, as OpenCV's copyTo(OutputArray) does
    void copyTo(Mat &&dst) const {
        CV_Assert(dst.rows == rows && dst.cols == cols && dst.type() == type_);
        for (int r = 0; r < rows; ++r) std::memcpy(dst.ptr(r), ptr(r), (size_t)cols * elemSize());
    }
    void copyTo(Mat &dst) const {
        dst.create(rows, cols, type_);
        for (int r = 0; r < rows; ++r) std::memcpy(dst.ptr(r), ptr(r), (size_t)cols * elemSize());
    }
    static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }   // create() zero-fills
    Mat t() const {
        Mat m(cols, rows, type_);
        const size_t es = elemSize();
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) std::memcpy(m.ptr(c) + r * es, ptr(r) + c * es, es);
        return m;
    }

    Mat rowRange(int r0, int r1) const {
        CV_Assert(0 <= r0 && r0 <= r1 && r1 <= rows);
        Mat m(*this);
        m.rows = r1 - r0; m.data = data ? data + (size_t)r0 * step : NULL;
        return m;
    }
    Mat colRange(int c0, int c1) const {
        CV_Assert(0 <= c0 && c0 <= c1 && c1 <= cols);
        Mat m(*this);
        m.cols = c1 - c0; m.data = data ? data + (size_t)c0 * elemSize() : NULL;
        return m;
    }
    Mat row(int r) const { return rowRange(r, r + 1); }
    Mat col(int c) const { return colRange(c, c + 1); }

    unsigned char *ptr(int r = 0) { return data + (size_t)r * step; }
    const unsigned char *ptr(int r = 0) const { return data + (size_t)r * step; }
    template <typename T> T *ptr(int r = 0) { return reinterpret_cast<T *>(ptr(r)); }
    template <typename T> const T *ptr(int r = 0) const { return reinterpret_cast<const T *>(ptr(r)); }

    template <typename T> T &at(int r, int c) { Check(r, c, sizeof(T)); return ptr<T>(r)[c]; }
    template <typename T> const T &at(int r, int c) const { Check(r, c, sizeof(T)); return ptr<T>(r)[c]; }
    // one index: a row vector, a column vector (a view may have a row step) or a continuous matrix, as OpenCV's Mat::at(int)
    template <typename T> T &at(int i) { int r, c; Split(i, r, c); return at<T>(r, c); }
    template <typename T> const T &at(int i) const { int r, c; Split(i, r, c); return at<T>(r, c); }

    double dot(const Mat &b) const {
        CV_Assert(type_ == CV_32F && b.type_ == CV_32F && total() == b.total());
        double s = 0.0;
        for (int i = 0; i < (int)total(); ++i) s += (double)Flat(i) * (double)b.Flat(i);
        return s;
    }

private:
    int type_;
    std::shared_ptr<std::vector<unsigned char> > buf_;

    static size_t ElemSize(int type) { return type == CV_32F ? 4 : 1; }
    void Check(int r, int c, size_t sz) const {
        CV_Assert(0 <= r && r < rows && 0 <= c && c < cols && sz == elemSize());
    }
    void Split(int i, int &r, int &c) const {
        if (rows == 1) { r = 0; c = i; }
        else if (cols == 1) { r = i; c = 0; }
        else { CV_Assert(cols > 0); r = i / cols; c = i % cols; }
    }
    float Flat(int i) const { return ptr<float>(i / cols)[i % cols]; }
};

typedef Mat MatExpr;

namespace detail {
inline Mat Like(const Mat &a) { CV_Assert(a.type() == CV_32F); return Mat(a.rows, a.cols, CV_32F); }
}  // namespace detail

inline Mat operator+(const Mat &a, const Mat &b) {
    CV_Assert(a.rows == b.rows && a.cols == b.cols);
    Mat m = detail::Like(a);
    for (int r = 0; r < a.rows; ++r) for (int c = 0; c < a.cols; ++c) m.at<float>(r, c) = a.at<float>(r, c) + b.at<float>(r, c);
    return m;
}
inline Mat operator-(const Mat &a, const Mat &b) {
    CV_Assert(a.rows == b.rows && a.cols == b.cols);
    Mat m = detail::Like(a);
    for (int r = 0; r < a.rows; ++r) for (int c = 0; c < a.cols; ++c) m.at<float>(r, c) = a.at<float>(r, c) - b.at<float>(r, c);
    return m;
}
inline Mat operator-(const Mat &a) {
    Mat m = detail::Like(a);
    for (int r = 0; r < a.rows; ++r) for (int c = 0; c < a.cols; ++c) m.at<float>(r, c) = -a.at<float>(r, c);
    return m;
}
inline Mat operator*(const Mat &a, double s) {
    Mat m = detail::Like(a);
    for (int r = 0; r < a.rows; ++r) for (int c = 0; c < a.cols; ++c) m.at<float>(r, c) = (float)((double)a.at<float>(r, c) * s);
    return m;
}
inline Mat operator*(double s, const Mat &a) { return a * s; }
inline Mat operator/(const Mat &a, double s) {
    Mat m = detail::Like(a);
    for (int r = 0; r < a.rows; ++r) for (int c = 0; c < a.cols; ++c) m.at<float>(r, c) = (float)((double)a.at<float>(r, c) / s);
    return m;
}
inline Mat operator*(const Mat &a, const Mat &b) {
    CV_Assert(a.type() == CV_32F && b.type() == CV_32F && a.cols == b.rows);
    Mat m(a.rows, b.cols, CV_32F);
    for (int i = 0; i < a.rows; ++i)
        for (int j = 0; j < b.cols; ++j) {
            double s = 0.0;
            for (int k = 0; k < a.cols; ++k) s += (double)a.at<float>(i, k) * (double)b.at<float>(k, j);
            m.at<float>(i, j) = (float)s;
        }
    return m;
}

inline double norm(const Mat &a) { return std::sqrt(a.dot(a)); }

class _InputArray {
public:
    _InputArray(const Mat &m) : m_(&m) {}
    Mat getMat() const { return *m_; }
    bool empty() const { return m_->empty(); }
private:
    const Mat *m_;
};
class _OutputArray {
public:
    _OutputArray(Mat &m) : m_(&m) {}
    Mat getMat() const { return *m_; }
    void create(int rows, int cols, int type) const { m_->create(rows, cols, type); }
    void release() const { m_->release(); }
private:
    Mat *m_;
};
typedef const _InputArray &InputArray;
typedef const _OutputArray &OutputArray;

}  // namespace cv
