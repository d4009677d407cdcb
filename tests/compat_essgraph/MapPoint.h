// tests/compat_essgraph: a MapPoint with the members compat/Optimizer_essentialgraph.inl touches (ORB-SLAM2 include/MapPoint.h:
// isBad, mnCorrectedByKF, mnCorrectedReference, GetReferenceKeyFrame, GetWorldPos, SetWorldPos) and the static member
// compat/MapPoint_batch.inl adds; here RefreshBatch only records what it was called with.
#pragma once
#include <vector>
#include <opencv2/core/core.hpp>
#include "KeyFrame.h"
namespace ORB_SLAM2 {
class MapPoint {
public:
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); ++nSetWorldPos; }
    bool isBad() { return mbBad; }
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }
    static void RefreshBatch(const std::vector<MapPoint *> &vpMPs, bool bDescriptors, bool bNormalAndDepth) {
        refreshed = vpMPs; refreshFlags = (bDescriptors ? 1 : 0) | (bNormalAndDepth ? 2 : 0);
    }
    cv::Mat mWorldPos;
    bool mbBad = false;
    KeyFrame *mpRefKF = NULL;
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    int nSetWorldPos = 0;
    static std::vector<MapPoint *> refreshed;
    static int refreshFlags;
};
}  // namespace ORB_SLAM2
