// tests/compat_localba: a KeyFrame with the members compat/Optimizer_localba.inl touches (ORB-SLAM2 include/KeyFrame.h: mnId,
// GetPose, SetPose, isBad, mvKeysUn, mvuRight, mvInvLevelSigma2, fx, fy, cx, cy, mbf, EraseMapPointMatch).  cv::Mat /
// cv::KeyPoint are the stand-ins of tests/compat_runtime/opencv2.
#pragma once
#include <utility>
#include <vector>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class MapPoint;
class KeyFrame {
public:
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat &T) { Tcw = T.clone(); ++nSetPose; }
    bool isBad() { return mbBad; }
    void EraseMapPointMatch(MapPoint *pMP) { erased.push_back(pMP); }
    long unsigned int mnId = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f, mbf = 0.f;
    cv::Mat Tcw;
    bool mbBad = false;
    int nSetPose = 0;
    std::vector<MapPoint *> erased;
};
}  // namespace ORB_SLAM2
