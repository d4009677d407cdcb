// tests/compat_localba/harness.cpp -- compat/Optimizer_localba.inl inside the function it belongs to, over the stand-ins of this
// directory, behind a C interface for tests/test_compat_localba.py (ctypes).  The three lists the reference collects at
// src/Optimizer.cc:636-708 come from the test.
#include <cstdint>
#include <cstring>
#include <list>
#include <map>
#include <mutex>
#include <stdexcept>
#include <vector>
#include "orbx.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "Map.h"

namespace ORB_SLAM2 {
using namespace std;
std::vector<MapPoint *> MapPoint::refreshed;
int MapPoint::refreshFlags = 0;

static void LocalBundleAdjustmentBody(KeyFrame *pKF, bool *pbStopFlag, Map *pMap, list<KeyFrame *> &lLocalKeyFrames,
                                      list<KeyFrame *> &lFixedCameras, list<MapPoint *> &lLocalMapPoints)
#include "Optimizer_localba.inl"
}  // namespace ORB_SLAM2

using namespace ORB_SLAM2;

// One scene from flat arrays (those of orbx_localba_problem; every observation is its own keypoint of its keyframe, with its own
// entry in the keyframe's level table).  bad_point: a point that reports isBad(), or -1 -- its erase entries are skipped.
// Returns the number of erased pairs, -1 when the fragment threw, -2 when the two erase calls did not come in pairs; Tcw_out
// [nlocal][16], world_out [npoints][3], erased [nobs] (1 where the pair was erased), info[0] = SetPose calls, info[1] = points
// handed to RefreshBatch, info[2] = its flags (1: descriptors, 2: normal and depth).
extern "C" int lba_compat_run(int nlocal, int nfixed, int npoints, const float *Tcw, const uint8_t *local_fixed, const float *camera,
                              float bf, const float *world, const int32_t *obs_begin, const int32_t *obs_kf, const float *obs,
                              const float *inv_sigma2, int stop, int bad_point, float *Tcw_out, float *world_out, uint8_t *erased,
                              int32_t *info) {
    const int nkf = nlocal + nfixed, nobs = obs_begin[npoints];
    std::vector<KeyFrame> kfs((size_t)nkf);
    std::vector<MapPoint> pts((size_t)npoints);
    for (int k = 0; k < nkf; ++k) {
        KeyFrame &K = kfs[(size_t)k];
        K.mnId = (k < nlocal && local_fixed[k]) ? 0 : (unsigned long)(k + 1);
        K.Tcw = cv::Mat(4, 4, CV_32F);
        std::memcpy(K.Tcw.ptr<float>(), Tcw + 16 * (size_t)k, 16 * sizeof(float));
        K.fx = camera[0]; K.fy = camera[1]; K.cx = camera[2]; K.cy = camera[3]; K.mbf = bf;
    }
    // the fragment walks std::map<KeyFrame *, size_t>: ascending keyframe address = ascending keyframe index here
    std::vector<std::vector<int> > edge_of((size_t)npoints);
    for (int p = 0; p < npoints; ++p) {
        MapPoint &M = pts[(size_t)p];
        M.mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; ++c) M.mWorldPos.at<float>(c) = world[3 * (size_t)p + c];
        M.mbBad = p == bad_point;
        for (int e = obs_begin[p]; e < obs_begin[p + 1]; ++e) {
            KeyFrame &K = kfs[(size_t)obs_kf[e]];
            cv::KeyPoint kp;
            kp.pt.x = obs[3 * (size_t)e]; kp.pt.y = obs[3 * (size_t)e + 1]; kp.octave = (int)K.mvInvLevelSigma2.size();
            K.mvKeysUn.push_back(kp); K.mvuRight.push_back(obs[3 * (size_t)e + 2]); K.mvInvLevelSigma2.push_back(inv_sigma2[e]);
            M.mObservations[&K] = K.mvKeysUn.size() - 1;
        }
    }
    std::list<KeyFrame *> lLocal, lFixed;
    std::list<MapPoint *> lPoints;
    for (int k = 0; k < nkf; ++k) (k < nlocal ? lLocal : lFixed).push_back(&kfs[(size_t)k]);
    for (int p = 0; p < npoints; ++p) lPoints.push_back(&pts[(size_t)p]);
    Map map;
    bool stopFlag = stop != 0;
    MapPoint::refreshed.clear(); MapPoint::refreshFlags = 0;
    try {
        LocalBundleAdjustmentBody(nkf ? &kfs[0] : NULL, &stopFlag, &map, lLocal, lFixed, lPoints);
    } catch (const std::exception &) {
        return -1;
    }
    int nerased = 0, nset = 0;
    std::memset(erased, 0, (size_t)nobs);
    for (int p = 0; p < npoints; ++p)
        for (int e = obs_begin[p]; e < obs_begin[p + 1]; ++e)
            if (!pts[(size_t)p].mObservations.count(&kfs[(size_t)obs_kf[e]])) { erased[e] = 1; ++nerased; }
    int nmatch = 0;
    for (int k = 0; k < nkf; ++k) { nmatch += (int)kfs[(size_t)k].erased.size(); nset += kfs[(size_t)k].nSetPose; }
    if (nmatch != nerased) return -2;                     // EraseMapPointMatch and EraseObservation come in pairs
    for (int k = 0; k < nlocal; ++k) std::memcpy(Tcw_out + 16 * (size_t)k, kfs[(size_t)k].Tcw.ptr<float>(), 16 * sizeof(float));
    for (int p = 0; p < npoints; ++p)
        for (int c = 0; c < 3; ++c) world_out[3 * (size_t)p + c] = pts[(size_t)p].mWorldPos.at<float>(c);
    info[0] = nset; info[1] = (int32_t)MapPoint::refreshed.size(); info[2] = MapPoint::refreshFlags;
    return nerased;
}
