// tests/compat_rgbd: a Frame with the members compat/Frame_rgbd.inl touches (ORB-SLAM2 include/Frame.h: mpORBextractorLeft, N,
// mvKeys, mvKeysUn, mvuRight, mvDepth, mbf).  Its one member function gets its body from compat/Frame_rgbd.inl (harness.cpp
// includes it).  cv::Mat / cv::KeyPoint are the stand-ins of tests/compat_runtime/opencv2.
#pragma once
#include <vector>
#include <opencv2/core/core.hpp>
#include "ORBextractor.h"
namespace ORB_SLAM2 {
class Frame {
public:
    void ComputeStereoFromRGBD(const cv::Mat &imDepth);
    ORBextractor *mpORBextractorLeft = NULL;
    float mbf = 0.f;
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
};
}  // namespace ORB_SLAM2
