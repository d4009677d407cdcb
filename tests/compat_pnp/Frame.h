// tests/compat_pnp: a Frame with the members compat/PnPsolver.h touches: mvKeysUn, mvLevelSigma2, mvpMapPoints and the static
// calibration floats fx, fy, cx, cy (defined in harness.cpp).
#pragma once
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapPoint.h"
namespace ORB_SLAM2 {
class Frame {
public:
    Frame(int levels, float scaleFactor) {
        float s = 1.f;
        for (int l = 0; l < levels; ++l) { mvLevelSigma2.push_back(s * s); s = s * scaleFactor; }
    }
    static float fx, fy, cx, cy;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
};
}  // namespace ORB_SLAM2
