// tests/compat_mappoint: the two MapPoint functions as single calls (rules in MapPoint.h), in the cv::Mat stand-in's arithmetic
#include <algorithm>
#include <climits>
#include <cstring>
#include "MapPoint.h"

namespace ORB_SLAM2 {

static int Hamming(const cv::Mat &a, const cv::Mat &b) {
    uint32_t wa[8], wb[8];
    std::memcpy(wa, a.ptr<uint8_t>(), 32);
    std::memcpy(wb, b.ptr<uint8_t>(), 32);
    int d = 0;
    for (int k = 0; k < 8; ++k) d += __builtin_popcount(wa[k] ^ wb[k]);
    return d;
}

void MapPoint::ComputeDistinctiveDescriptors() {
    std::map<KeyFrame *, size_t> obs;
    {
        std::unique_lock<std::mutex> lock(mMutexFeatures);
        if (mbBad) return;
        obs = mObservations;
    }
    std::vector<cv::Mat> d;
    for (std::map<KeyFrame *, size_t>::iterator it = obs.begin(); it != obs.end(); ++it)
        if (!it->first->isBad()) d.push_back(it->first->mDescriptors.row((int)it->second));
    if (d.empty()) return;
    const size_t n = d.size();
    int bestMedian = INT_MAX;
    size_t bestIdx = 0;
    std::vector<int> row(n);
    for (size_t i = 0; i < n; ++i) {
        for (size_t j = 0; j < n; ++j) row[j] = i == j ? 0 : Hamming(d[i], d[j]);
        std::sort(row.begin(), row.end());
        const int median = row[(n - 1) / 2];
        if (median < bestMedian) { bestMedian = median; bestIdx = i; }
    }
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    mDescriptor = d[bestIdx].clone();
}

void MapPoint::UpdateNormalAndDepth() {
    std::map<KeyFrame *, size_t> obs;
    KeyFrame *pRefKF;
    cv::Mat Pos;
    {
        std::unique_lock<std::mutex> lock1(mMutexFeatures);
        std::unique_lock<std::mutex> lock2(mMutexPos);
        if (mbBad) return;
        obs = mObservations;
        pRefKF = mpRefKF;
        Pos = mWorldPos.clone();
    }
    if (obs.empty()) return;
    cv::Mat normal = cv::Mat::zeros(3, 1, CV_32F);
    int n = 0;
    for (std::map<KeyFrame *, size_t>::iterator it = obs.begin(); it != obs.end(); ++it) {
        const cv::Mat di = Pos - it->first->GetCameraCenter();
        normal = normal + di / cv::norm(di);
        ++n;
    }
    const cv::Mat PC = Pos - pRefKF->GetCameraCenter();
    const float dist = (float)cv::norm(PC);
    const int level = pRefKF->mvKeysUn[obs[pRefKF]].octave;
    const float levelScaleFactor = pRefKF->mvScaleFactors[level];
    const int nLevels = pRefKF->mnScaleLevels;
    std::unique_lock<std::mutex> lock3(mMutexPos);
    mfMaxDistance = dist * levelScaleFactor;
    mfMinDistance = mfMaxDistance / pRefKF->mvScaleFactors[nLevels - 1];
    mNormalVector = normal / n;
}

}  // namespace ORB_SLAM2
