// tests/compat_sim3: a KeyFrame with the members compat/Sim3Solver.h touches: the slot vector (NULL and bad points included),
// copies of Rcw and tcw, mvKeysUn, mvLevelSigma2 and the calibration matrix mK.
#pragma once
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapPoint.h"
namespace ORB_SLAM2 {
class KeyFrame {
public:
    KeyFrame(const cv::Mat &Tcw_, const float *K4, int levels, float scaleFactor) : Tcw(Tcw_.clone()), mK(3, 3, CV_32F) {
        mK.at<float>(0, 0) = K4[0]; mK.at<float>(1, 1) = K4[1]; mK.at<float>(0, 2) = K4[2]; mK.at<float>(1, 2) = K4[3];
        mK.at<float>(2, 2) = 1.f;
        float s = 1.f;
        for (int l = 0; l < levels; ++l) { mvLevelSigma2.push_back(s * s); s = s * scaleFactor; }
    }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    cv::Mat GetRotation() { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }
    cv::Mat GetTranslation() { return Tcw.rowRange(0, 3).col(3).clone(); }

    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
private:
    cv::Mat Tcw;
public:
    cv::Mat mK;
};
}  // namespace ORB_SLAM2
