// oracle/ref/extractor: the cv:: that the reference's src/ORBextractor.cc is compiled against, unmodified.
//
// This cv:: holds NO ALGORITHM OF ITS OWN.  cv::Mat is a reference-counted byte buffer with views; the six OpenCV primitives
// forward to the oracle's restatements (oracle/orb_oracle.h), which are therefore the same on both sides of every comparison
// and stay unpinned:
//
//     FAST            -> orc_fast9_16            (TYPE_9_16, nonmaxSuppression = true only)
//     resize          -> orc_resize_linear_u8    (INTER_LINEAR with an explicit dsize only)
//     copyMakeBorder  -> orc_border_reflect101   (BORDER_REFLECT_101, with or without BORDER_ISOLATED, equal borders only)
//     GaussianBlur    -> orc_gaussian_blur7      (7 x 7, sigma 2 / 2, BORDER_REFLECT_101 only)
//     fastAtan2       -> orc_fast_atan2
//     cvRound         -> half to even (lrint / lrintf under the default rounding mode), as OpenCV's SSE2 cvtsd2si / cvtss2si
//
// Every argument combination outside that list aborts with a message, so this file documents exactly what it stands for.
// Only CV_8UC1 exists.
#pragma once
#include <algorithm>   // OpenCV's own core.hpp brings the standard headers the reference relies on
#include <cassert>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "orb_oracle.h"

#define CV_8U 0
#define CV_8UC1 0
#define CV_PI 3.1415926535897932384626433832795

namespace cv {

typedef unsigned char uchar;

[[noreturn]] inline void standin_abort(const char *what)
{
    std::fprintf(stderr, "oracle/ref/extractor cv:: stand-in: %s\n", what);
    std::abort();
}

inline int cvRound(double v) { return (int)lrint(v); }
inline int cvRound(float v) { return (int)lrintf(v); }
inline int cvRound(int v) { return v; }
inline int cvFloor(double v) { int i = (int)v; return i - (i > v); }
inline int cvFloor(float v) { int i = (int)v; return i - (i > v); }
inline int cvCeil(double v) { int i = (int)v; return i + (i < v); }
inline int cvCeil(float v) { int i = (int)v; return i + (i < v); }
inline float fastAtan2(float y, float x) { return orc_fast_atan2(y, x); }

template <typename T> struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T _x, T _y) : x(_x), y(_y) {}
};
typedef Point_<int> Point2i;
typedef Point_<int> Point;
typedef Point_<float> Point2f;
// OpenCV: a.x = saturate_cast<float>(a.x * b), which for float operands is the plain product
inline Point2f &operator*=(Point2f &a, float b) { a.x = a.x * b; a.y = a.y * b; return a; }

struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};
struct Rect {
    int x, y, width, height;
    Rect() : x(0), y(0), width(0), height(0) {}
    Rect(int _x, int _y, int w, int h) : x(_x), y(_y), width(w), height(h) {}
};
struct Scalar {
    double val[4];
    Scalar() { val[0] = val[1] = val[2] = val[3] = 0; }
};

struct KeyPoint {            // bit-compatible with orc_keypoint and with OpenCV's 28-byte cv::KeyPoint
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
    KeyPoint() : pt(0, 0), size(0), angle(-1), response(0), octave(0), class_id(-1) {}
};
static_assert(sizeof(KeyPoint) == 28 && sizeof(KeyPoint) == sizeof(orc_keypoint), "cv::KeyPoint layout");

struct KeyPointsFilter {     // only ComputeKeyPointsOld, which nothing calls, uses it
    static void retainBest(std::vector<KeyPoint> &, int) { standin_abort("KeyPointsFilter::retainBest is not implemented"); }
};

enum { INTER_NEAREST = 0, INTER_LINEAR = 1, INTER_CUBIC = 2, INTER_AREA = 3 };
enum { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_WRAP = 3, BORDER_REFLECT_101 = 4,
       BORDER_REFLECT101 = 4, BORDER_DEFAULT = 4, BORDER_ISOLATED = 16 };

struct MatStep {
    size_t v;
    MatStep() : v(0) {}
    MatStep(size_t s) : v(s) {}
    operator size_t() const { return v; }
};

struct MatExpr {             // Mat::zeros: assigning it to a Mat of the same size and type fills that Mat's buffer in place
    int rows, cols, type;
};

class Mat {
    struct Buf { uchar *mem; int refs; };
    Buf *buf;                // null for an empty Mat and for a header over caller-owned memory
    void retain() { if (buf) ++buf->refs; }
    void drop()
    {
        if (buf && --buf->refs == 0) { std::free(buf->mem); delete buf; }
        buf = 0;
    }
    static void check_type(int type) { if (type != CV_8UC1) standin_abort("only CV_8UC1 matrices are implemented"); }

public:
    int rows, cols;
    uchar *data;
    MatStep step;
    bool sub;                // a view smaller than the matrix it was taken from (OpenCV: isSubmatrix())

    Mat() : buf(0), rows(0), cols(0), data(0), step(0), sub(false) {}
    Mat(int r, int c, int type) : buf(0), rows(0), cols(0), data(0), step(0), sub(false) { create(r, c, type); }
    Mat(Size s, int type) : buf(0), rows(0), cols(0), data(0), step(0), sub(false) { create(s.height, s.width, type); }
    Mat(int r, int c, int type, void *d, size_t st) : buf(0), rows(r), cols(c), data((uchar *)d), step(st), sub(false) { check_type(type); }
    Mat(const Mat &m) : buf(m.buf), rows(m.rows), cols(m.cols), data(m.data), step(m.step), sub(m.sub) { retain(); }
    Mat(const MatExpr &e) : buf(0), rows(0), cols(0), data(0), step(0), sub(false) { *this = e; }
    ~Mat() { drop(); }
    Mat &operator=(const Mat &m)
    {
        if (this != &m) {
            Buf *old = buf;
            buf = m.buf; retain();
            rows = m.rows; cols = m.cols; data = m.data; step = m.step; sub = m.sub;
            if (old && --old->refs == 0) { std::free(old->mem); delete old; }
        }
        return *this;
    }
    Mat &operator=(const MatExpr &e)
    {
        create(e.rows, e.cols, e.type);
        for (int y = 0; y < rows; ++y) std::memset(data + (size_t)y * step, 0, (size_t)cols);
        return *this;
    }
    // OpenCV's Mat::create: a matrix that already has this size and type keeps its buffer (a view stays a view)
    void create(int r, int c, int type)
    {
        check_type(type);
        if (r < 0 || c < 0) standin_abort("Mat::create with a negative size");
        if (data && rows == r && cols == c) return;
        drop();
        rows = r; cols = c; step = (size_t)c; sub = false; data = 0;
        if (r > 0 && c > 0) {
            buf = new Buf;
            buf->mem = (uchar *)std::malloc((size_t)r * c);
            if (!buf->mem) standin_abort("out of memory");
            buf->refs = 1;
            data = buf->mem;
        }
    }
    void create(Size s, int type) { create(s.height, s.width, type); }
    void release() { drop(); rows = cols = 0; data = 0; step = 0; sub = false; }
    Mat operator()(const Rect &r) const
    {
        if (r.x < 0 || r.y < 0 || r.width < 0 || r.height < 0 || r.x + r.width > cols || r.y + r.height > rows)
            standin_abort("Mat::operator()(Rect) outside the matrix");
        Mat m(*this);
        m.data = data + (size_t)r.y * step + r.x;
        m.rows = r.height; m.cols = r.width;
        m.sub = sub || r.width < cols || r.height < rows;
        return m;
    }
    Mat rowRange(int a, int b) const { return (*this)(Rect(0, a, cols, b - a)); }
    Mat colRange(int a, int b) const { return (*this)(Rect(a, 0, b - a, rows)); }
    Mat clone() const
    {
        Mat m(rows, cols, CV_8UC1);
        for (int y = 0; y < rows; ++y) std::memcpy(m.data + (size_t)y * m.step, data + (size_t)y * step, (size_t)cols);
        return m;
    }
    static MatExpr zeros(int r, int c, int type) { MatExpr e = {r, c, type}; return e; }
    bool empty() const { return data == 0 || rows == 0 || cols == 0; }
    int type() const { return CV_8UC1; }
    size_t step1() const { return step; }
    bool isSubmatrix() const { return sub; }
    bool shares(const Mat &o) const { return buf && buf == o.buf; }
    uchar *ptr(int y = 0) { return data + (size_t)y * step; }
    const uchar *ptr(int y = 0) const { return data + (size_t)y * step; }
    template <typename T> T &at(int y, int x) { static_assert(sizeof(T) == 1, "8UC1 only"); return *(T *)(data + (size_t)y * step + x); }
    template <typename T> const T &at(int y, int x) const { static_assert(sizeof(T) == 1, "8UC1 only"); return *(const T *)(data + (size_t)y * step + x); }
};

class _InputArray {
protected:
    Mat *m;
public:
    _InputArray() : m(0) {}
    _InputArray(const Mat &mat) : m(const_cast<Mat *>(&mat)) {}
    bool empty() const { return !m || m->empty(); }
    Mat getMat() const { return m ? *m : Mat(); }
};
class _OutputArray : public _InputArray {
public:
    _OutputArray() {}
    _OutputArray(Mat &mat) : _InputArray(mat) {}
    void create(int r, int c, int type) const { if (!m) standin_abort("OutputArray without a Mat"); m->create(r, c, type); }
    void create(Size s, int type) const { create(s.height, s.width, type); }
    void release() const { if (m) m->release(); }
};
typedef const _InputArray &InputArray;
typedef const _OutputArray &OutputArray;

// ---- the forwards.  fast_hook, when set, sees every FAST call (image view, threshold, what it returned): the harness records
// the candidates with their level through it.
typedef void (*fast_hook_t)(const Mat &image, int threshold, const std::vector<KeyPoint> &keypoints);
inline fast_hook_t &fast_hook() { static fast_hook_t h = 0; return h; }

inline void FAST(InputArray _image, std::vector<KeyPoint> &keypoints, int threshold, bool nonmaxSuppression = true)
{
    if (!nonmaxSuppression) standin_abort("FAST without non-maximum suppression is not implemented");
    Mat image = _image.getMat();
    keypoints.clear();
    if (!image.empty()) {
        int cap = image.rows * image.cols;
        std::vector<orc_keypoint> out((size_t)cap);
        int n = orc_fast9_16(image.data, image.cols, image.rows, (int)(size_t)image.step, threshold, out.data(), cap);
        if (n > cap) standin_abort("FAST returned more corners than pixels");
        keypoints.resize((size_t)n);
        if (n) std::memcpy(keypoints.data(), out.data(), (size_t)n * sizeof(KeyPoint));
    }
    if (fast_hook()) fast_hook()(image, threshold, keypoints);
}

inline void resize(InputArray _src, OutputArray _dst, Size dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR)
{
    if (interpolation != INTER_LINEAR) standin_abort("resize: only INTER_LINEAR is implemented");
    if (dsize.width <= 0 || dsize.height <= 0 || fx != 0 || fy != 0) standin_abort("resize: only an explicit dsize (fx = fy = 0) is implemented");
    Mat src = _src.getMat();
    if (src.empty()) standin_abort("resize of an empty matrix");
    _dst.create(dsize, src.type());
    Mat dst = _dst.getMat();
    if (dst.shares(src)) standin_abort("resize within one buffer is not implemented");
    orc_resize_linear_u8(src.data, src.cols, src.rows, (int)(size_t)src.step, dst.data, dst.cols, dst.rows, (int)(size_t)dst.step);
}

inline void copyMakeBorder(InputArray _src, OutputArray _dst, int top, int bottom, int left, int right, int borderType,
                           const Scalar & = Scalar())
{
    if ((borderType & ~BORDER_ISOLATED) != BORDER_REFLECT_101) standin_abort("copyMakeBorder: only BORDER_REFLECT_101 (+ BORDER_ISOLATED) is implemented");
    if (top != bottom || top != left || top != right || top < 0) standin_abort("copyMakeBorder: only four equal borders are implemented");
    Mat src = _src.getMat();
    if (src.empty()) standin_abort("copyMakeBorder of an empty matrix");
    // without BORDER_ISOLATED OpenCV reads the border of a submatrix from the pixels around it; that is not implemented
    if (!(borderType & BORDER_ISOLATED) && src.isSubmatrix()) standin_abort("copyMakeBorder: a submatrix source needs BORDER_ISOLATED");
    _dst.create(src.rows + 2 * top, src.cols + 2 * top, src.type());
    Mat dst = _dst.getMat();
    if (dst.shares(src)) {   // in place (the fork: the ROI of temp into temp): the source must be exactly the interior
        if (src.data != dst.data + (size_t)top * dst.step + top || (size_t)src.step != (size_t)dst.step)
            standin_abort("copyMakeBorder: an in-place source must be the interior of the destination");
        Mat copy = src.clone();
        orc_border_reflect101(copy.data, copy.cols, copy.rows, (int)(size_t)copy.step, dst.data, (int)(size_t)dst.step, top);
    } else
        orc_border_reflect101(src.data, src.cols, src.rows, (int)(size_t)src.step, dst.data, (int)(size_t)dst.step, top);
}

inline void GaussianBlur(InputArray _src, OutputArray _dst, Size ksize, double sigmaX, double sigmaY = 0, int borderType = BORDER_DEFAULT)
{
    if (ksize.width != 7 || ksize.height != 7 || sigmaX != 2 || sigmaY != 2) standin_abort("GaussianBlur: only 7 x 7 with sigma 2 / 2 is implemented");
    if (borderType != BORDER_REFLECT_101) standin_abort("GaussianBlur: only BORDER_REFLECT_101 is implemented");
    Mat src = _src.getMat();
    if (src.empty()) standin_abort("GaussianBlur of an empty matrix");
    if (src.isSubmatrix()) standin_abort("GaussianBlur of a submatrix (OpenCV would read around it) is not implemented");
    _dst.create(src.rows, src.cols, src.type());
    Mat dst = _dst.getMat();
    if (dst.data == src.data) {          // in place, as the fork calls it
        Mat copy = src.clone();
        orc_gaussian_blur7(copy.data, copy.cols, copy.rows, (int)(size_t)copy.step, dst.data, (int)(size_t)dst.step);
    } else
        orc_gaussian_blur7(src.data, src.cols, src.rows, (int)(size_t)src.step, dst.data, (int)(size_t)dst.step);
}

}  // namespace cv
