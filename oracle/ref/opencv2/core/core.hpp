// oracle/ref: the part of <opencv2/core/core.hpp> that the reference's DBoW2 (BowVector, ScoringObject, FeatureVector, FORB,
// TemplatedVocabulary) and KeyFrameDatabase.cc need in order to compile unmodified.  Written here; no OpenCV text.
//   cv::Mat          a container only: create / release / clone / ptr<T> / zeros / rows / cols, single channel CV_8U or CV_32F,
//                    rows stored one after the other, zero-filled on creation (FORB::fromString relies on no arithmetic)
//   cv::FileStorage  inert: never opened, every write is dropped, every read yields an empty cv::FileNode.  The YAML
//   cv::FileNode     save / load of the vocabulary compile against them and are never called; the text loader is used.
// The real header pulls in <cmath>, <sstream> and <iostream>, which the reference's sources rely on (::pow, ::log, std::cerr);
// so does this one.
#pragma once
#include <math.h>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_32F 5

namespace cv {

class Mat {
public:
    int rows, cols;
    unsigned char *data;

    Mat() : rows(0), cols(0), data(NULL), type_(CV_8U) {}
    Mat(int r, int c, int type) : rows(0), cols(0), data(NULL), type_(CV_8U) { create(r, c, type); }

    static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }   // create() zero-fills

    void create(int r, int c, int type) {
        if (data && rows == r && cols == c && type_ == type) return;
        if (r < 0 || c < 0 || (type != CV_8U && type != CV_32F)) throw std::runtime_error("oracle/ref cv::Mat: unsupported create");
        type_ = type; rows = r; cols = c;
        buf_ = std::make_shared<std::vector<unsigned char> >((size_t)r * c * (type == CV_32F ? 4 : 1) + 1, 0);
        data = buf_->data();
    }
    void release() { buf_.reset(); data = NULL; rows = cols = 0; }
    Mat clone() const {
        Mat m(rows, cols, type_);
        if (data) std::memcpy(m.data, data, (size_t)rows * cols * (type_ == CV_32F ? 4 : 1));
        return m;
    }
    int type() const { return type_; }
    bool empty() const { return data == NULL || rows == 0 || cols == 0; }

    template <typename T> T *ptr(int r = 0) { return reinterpret_cast<T *>(data + (size_t)r * cols * (type_ == CV_32F ? 4 : 1)); }
    template <typename T> const T *ptr(int r = 0) const {
        return reinterpret_cast<const T *>(data + (size_t)r * cols * (type_ == CV_32F ? 4 : 1));
    }

private:
    int type_;
    std::shared_ptr<std::vector<unsigned char> > buf_;
};

class FileNode {
public:
    FileNode operator[](const std::string &) const { return FileNode(); }
    FileNode operator[](const char *) const { return FileNode(); }
    FileNode operator[](int) const { return FileNode(); }
    size_t size() const { return 0; }
    operator int() const { return 0; }
    operator double() const { return 0.0; }
    operator std::string() const { return std::string(); }
};

class FileStorage {
public:
    enum { READ = 0, WRITE = 1 };
    FileStorage() {}
    FileStorage(const std::string &, int) {}
    bool isOpened() const { return false; }
    FileNode operator[](const std::string &) const { return FileNode(); }
    FileNode operator[](const char *) const { return FileNode(); }
};
template <typename T> inline FileStorage &operator<<(FileStorage &fs, const T &) { return fs; }

}  // namespace cv
