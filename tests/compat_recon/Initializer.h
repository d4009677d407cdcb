// tests/compat_recon: an Initializer with the members compat/Initializer_reconstruct.inl touches -- mvKeys1, mvKeys2, mvMatches12,
// mSigma, with the reference's types (include/Initializer.h:46, :311-338) -- and the two member functions whose bodies the
// fragment is, with the reference's signatures (:963-971, :1154-1161).  cv::Point3f is not in tests/compat_runtime's cv, so it is
// defined here.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>
#include <opencv2/core/core.hpp>
#include "orbx.h"
namespace cv {
struct Point3f {
    float x, y, z;
    Point3f() : x(0.f), y(0.f), z(0.f) {}
    Point3f(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};
}  // namespace cv
namespace ORB_SLAM2 {
using namespace std;
class Initializer {
    typedef pair<int, int> Match;
public:
    Initializer(float sigma) : mSigma(sigma), mSigma2(sigma * sigma) {}
    bool ReconstructF(vector<bool> &vbMatchesInliers, cv::Mat &F21, cv::Mat &K, cv::Mat &R21, cv::Mat &t21, vector<cv::Point3f> &vP3D,
                      vector<bool> &vbTriangulated, float minParallax, int minTriangulated)
    {
#define ORBX_RECONSTRUCT_MODEL ORBX_INIT_F
#define ORBX_RECONSTRUCT_MATRIX F21
#include "Initializer_reconstruct.inl"
    }
    bool ReconstructH(vector<bool> &vbMatchesInliers, cv::Mat &H21, cv::Mat &K, cv::Mat &R21, cv::Mat &t21, vector<cv::Point3f> &vP3D,
                      vector<bool> &vbTriangulated, float minParallax, int minTriangulated)
    {
#define ORBX_RECONSTRUCT_MODEL ORBX_INIT_H
#define ORBX_RECONSTRUCT_MATRIX H21
#include "Initializer_reconstruct.inl"
    }
    vector<cv::KeyPoint> mvKeys1;
    vector<cv::KeyPoint> mvKeys2;
    vector<Match> mvMatches12;
    float mSigma, mSigma2;
};
}  // namespace ORB_SLAM2
