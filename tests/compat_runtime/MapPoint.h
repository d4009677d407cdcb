// tests/compat_runtime: a working MapPoint with the members compat/ORBmatcher.h touches (the member list of
// tests/compat_stubs/MapPoint.h) and the map rules of ORB-SLAM2's MapPoint, restated (bodies in map_model.cpp):
//   AddObservation(kf, i)   ignored when kf already observes the point; otherwise records slot i and adds 2 to the
//                           observation count when kf->mvuRight[i] >= 0 (a stereo observation), else 1 (src/MapPoint.cc:175-193)
//   Replace(other)          no-op on itself; otherwise takes this point's observations, clears them and marks it bad (its count
//                           is left as it was); for each former keyframe the slot goes to `other` (ReplaceMapPointMatch + other's
//                           AddObservation) unless `other` already observes that keyframe, in which case the slot is emptied
//                           (EraseMapPointMatch); then other->ComputeDistinctiveDescriptors() (:300-374)
//   ComputeDistinctiveDescriptors   nothing for a bad or unobserved point; otherwise the observing keyframes' descriptor rows,
//                           in observation order, the pairwise Hamming distances, and the row whose sorted distances have the
//                           smallest element at index (N-1)/2 -- the first such row on a tie (:424-516)
//   PredictScale(d, kf|F)   ceil(log(mfMaxDistance / d) / mfLogScaleFactor), clamped to [0, levels-1] (:676-722)
//   Min/MaxDistanceInvariance   0.8 * mfMinDistance and 1.2 * mfMaxDistance (:640-650)
//   SetBadFlag              marks the point bad and empties its slots in every observing keyframe (:256-287)
// Observations are kept in keyframe-id order.  The reference keys them by KeyFrame pointer, which orders them by allocation
// address; ids give the same kind of fixed order, reproducibly.  There are no locks: the harness is single-threaded.
#pragma once
#include <map>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class Frame;
struct KeyFrameIdLess { bool operator()(const KeyFrame *a, const KeyFrame *b) const; };
class MapPoint {
public:
    MapPoint(long unsigned int id, const cv::Mat &pos, const cv::Mat &normal, const cv::Mat &desc, float minDist, float maxDist)
        : mnId(id), mWorldPos(pos.clone()), mNormalVector(normal.clone()), mDescriptor(desc.clone()), mfMinDistance(minDist),
          mfMaxDistance(maxDist) {}

    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    int Observations() { return nObs; }
    bool isBad() { return mbBad; }
    bool IsInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) != 0; }
    int GetIndexInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
    std::map<KeyFrame *, size_t, KeyFrameIdLess> GetObservations() { return mObservations; }
    void AddObservation(KeyFrame *pKF, size_t idx);
    void Replace(MapPoint *pMP);
    void SetBadFlag();
    void ComputeDistinctiveDescriptors();
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    int PredictScale(const float &currentDist, KeyFrame *pKF);
    int PredictScale(const float &currentDist, Frame *pF);

    long unsigned int mnId;
    float mTrackProjX = 0.f, mTrackProjY = 0.f, mTrackProjXR = 0.f;
    bool mbTrackInView = false;
    int mnTrackScaleLevel = 0;
    float mTrackViewCos = 0.f;
    long unsigned int mnLastFrameSeen = 0;

private:
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistance, mfMaxDistance;
    std::map<KeyFrame *, size_t, KeyFrameIdLess> mObservations;
    int nObs = 0;
    bool mbBad = false;
};
}  // namespace ORB_SLAM2
