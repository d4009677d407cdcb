// tests/compat_localba: a MapPoint with the members compat/Optimizer_localba.inl touches (ORB-SLAM2 include/MapPoint.h:
// GetWorldPos, SetWorldPos, GetObservations, isBad, EraseObservation) and the static member compat/MapPoint_batch.inl adds;
// here RefreshBatch only records what it was called with.
#pragma once
#include <map>
#include <vector>
#include <opencv2/core/core.hpp>
#include "KeyFrame.h"
namespace ORB_SLAM2 {
class MapPoint {
public:
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    bool isBad() { return mbBad; }
    void EraseObservation(KeyFrame *pKF) { mObservations.erase(pKF); }
    static void RefreshBatch(const std::vector<MapPoint *> &vpMPs, bool bDescriptors, bool bNormalAndDepth) {
        refreshed = vpMPs; refreshFlags = (bDescriptors ? 1 : 0) | (bNormalAndDepth ? 2 : 0);
    }
    cv::Mat mWorldPos;
    std::map<KeyFrame *, size_t> mObservations;
    bool mbBad = false;
    static std::vector<MapPoint *> refreshed;
    static int refreshFlags;
};
}  // namespace ORB_SLAM2
