// tests/compat_sim3: a MapPoint with the members compat/Sim3Solver.h touches: isBad, GetWorldPos, GetIndexInKeyFrame (the slot
// of the point in a keyframe, -1 when the keyframe does not observe it, src/MapPoint.cc:289-297).
#pragma once
#include <map>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
public:
    MapPoint(const cv::Mat &pos, bool bad) : mWorldPos(pos.clone()), mbBad(bad) {}
    bool isBad() { return mbBad; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    int GetIndexInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) ? mObservations[pKF] : -1; }
    void AddObservation(KeyFrame *pKF, int idx) { mObservations[pKF] = idx; }
private:
    cv::Mat mWorldPos;
    bool mbBad;
    std::map<KeyFrame *, int> mObservations;
};
}  // namespace ORB_SLAM2
