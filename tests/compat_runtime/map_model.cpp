// tests/compat_runtime: the MapPoint bodies (rules in MapPoint.h) and Frame's static image bounds
#include <algorithm>
#include <climits>
#include <cmath>
#include "MapPoint.h"
#include "KeyFrame.h"
#include "Frame.h"
#include "ORBmatcher.h"

namespace ORB_SLAM2 {

float Frame::mnMinX = 0.f, Frame::mnMaxX = 0.f, Frame::mnMinY = 0.f, Frame::mnMaxY = 0.f;

bool KeyFrameIdLess::operator()(const KeyFrame *a, const KeyFrame *b) const { return a->mnId < b->mnId; }

void MapPoint::AddObservation(KeyFrame *pKF, size_t idx) {
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    nObs += pKF->mvuRight.at(idx) >= 0 ? 2 : 1;
}

void MapPoint::SetBadFlag() {
    mbBad = true;
    const std::map<KeyFrame *, size_t, KeyFrameIdLess> obs = mObservations;
    mObservations.clear();
    for (auto it = obs.begin(); it != obs.end(); ++it) it->first->EraseMapPointMatch(it->second);
}

void MapPoint::Replace(MapPoint *pMP) {
    if (pMP->mnId == mnId) return;
    const std::map<KeyFrame *, size_t, KeyFrameIdLess> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    for (auto it = obs.begin(); it != obs.end(); ++it) {
        KeyFrame *pKF = it->first;
        if (!pMP->IsInKeyFrame(pKF)) {
            pKF->ReplaceMapPointMatch(it->second, pMP);
            pMP->AddObservation(pKF, it->second);
        } else {
            pKF->EraseMapPointMatch(it->second);
        }
    }
    pMP->ComputeDistinctiveDescriptors();
}

void MapPoint::ComputeDistinctiveDescriptors() {
    if (mbBad || mObservations.empty()) return;
    std::vector<cv::Mat> d;
    for (auto it = mObservations.begin(); it != mObservations.end(); ++it)
        if (!it->first->isBad()) d.push_back(it->first->mDescriptors.row((int)it->second));
    if (d.empty()) return;
    const size_t n = d.size();
    std::vector<std::vector<int> > dist(n, std::vector<int>(n, 0));
    for (size_t i = 0; i < n; ++i)
        for (size_t j = i + 1; j < n; ++j) dist[i][j] = dist[j][i] = ORBmatcher::DescriptorDistance(d[i], d[j]);
    int bestMedian = INT_MAX;
    size_t bestIdx = 0;
    for (size_t i = 0; i < n; ++i) {
        std::vector<int> row = dist[i];
        std::sort(row.begin(), row.end());
        const int median = row[(n - 1) / 2];
        if (median < bestMedian) { bestMedian = median; bestIdx = i; }
    }
    mDescriptor = d[bestIdx].clone();
}

static int ClampedScale(float maxDistance, float currentDist, float logScaleFactor, int levels) {
    const float ratio = maxDistance / currentDist;
    int nScale = (int)std::ceil(std::log(ratio) / logScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= levels) nScale = levels - 1;
    return nScale;
}
int MapPoint::PredictScale(const float &currentDist, KeyFrame *pKF) {
    return ClampedScale(mfMaxDistance, currentDist, pKF->mfLogScaleFactor, pKF->mnScaleLevels);
}
int MapPoint::PredictScale(const float &currentDist, Frame *pF) {
    return ClampedScale(mfMaxDistance, currentDist, pF->mfLogScaleFactor, pF->mnScaleLevels);
}

}  // namespace ORB_SLAM2
