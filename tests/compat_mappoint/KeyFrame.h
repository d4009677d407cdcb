// tests/compat_mappoint: a KeyFrame with the members compat/MapPoint_batch.inl and the two MapPoint functions touch (ORB-SLAM2
// include/KeyFrame.h: mnId, mDescriptors, mvKeysUn, mfScaleFactor, mnScaleLevels, mvScaleFactors, isBad, GetCameraCenter).
// cv::Mat / cv::KeyPoint are the stand-ins of tests/compat_runtime/opencv2.
#pragma once
#include <vector>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame {
public:
    bool isBad() { return mbBad; }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    long unsigned int mnId = 0;
    cv::Mat mDescriptors;
    std::vector<cv::KeyPoint> mvKeysUn;
    float mfScaleFactor = 1.2f;
    int mnScaleLevels = 8;
    std::vector<float> mvScaleFactors;
    cv::Mat Ow;
    bool mbBad = false;
};
}  // namespace ORB_SLAM2
