// tests/compat_pnp: a MapPoint with the members compat/PnPsolver.h touches: isBad and GetWorldPos.
#pragma once
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class MapPoint {
public:
    MapPoint(const cv::Mat &pos, bool bad) : mWorldPos(pos.clone()), mbBad(bad) {}
    bool isBad() { return mbBad; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
private:
    cv::Mat mWorldPos;
    bool mbBad;
};
}  // namespace ORB_SLAM2
