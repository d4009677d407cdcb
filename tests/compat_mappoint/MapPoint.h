// tests/compat_mappoint: a MapPoint with the members the two refresh functions read and write (ORB-SLAM2 include/MapPoint.h), the
// two functions themselves restated in map_model.cpp (the loop tests/test_compat_mappoint.py compares with), and the static
// member the maintainer declares for compat/MapPoint_batch.inl (harness.cpp includes its body).  Rules of the restatement:
//   ComputeDistinctiveDescriptors   nothing for a bad or unobserved point; otherwise the rows of the keyframes that are not bad,
//                                   in the map's order (std::map<KeyFrame*, size_t>: by address); nothing when none is left;
//                                   the row whose median distance to all rows (itself included, element (N - 1) / 2 of the
//                                   sorted row) is smallest, the first of equal ones (src/MapPoint.cc:424-516)
//   UpdateNormalAndDepth            nothing for a bad or unobserved point; otherwise normal = sum over ALL observing keyframes in
//                                   the map's order of (Pos - Ow_i) / norm(Pos - Ow_i), dist = norm(Pos - Ow_ref),
//                                   mfMaxDistance = dist * mvScaleFactors[octave of the point's keypoint in the reference
//                                   keyframe], mfMinDistance = mfMaxDistance / mvScaleFactors[nLevels - 1], mNormalVector =
//                                   normal / n, in cv::Mat's arithmetic (:570-638)
#pragma once
#include <map>
#include <mutex>
#include <vector>
#include <opencv2/core/core.hpp>
#include "KeyFrame.h"
namespace ORB_SLAM2 {
class MapPoint {
public:
    void ComputeDistinctiveDescriptors();
    void UpdateNormalAndDepth();
    static void RefreshBatch(const std::vector<MapPoint *> &vpMPs, bool bDescriptors, bool bNormalAndDepth);

    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    std::map<KeyFrame *, size_t> mObservations;
    KeyFrame *mpRefKF = NULL;
    float mfMinDistance = 0.f, mfMaxDistance = 0.f;
    bool mbBad = false;
    std::mutex mMutexPos, mMutexFeatures;
};
}  // namespace ORB_SLAM2
