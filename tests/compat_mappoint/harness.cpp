// tests/compat_mappoint: extern "C" entry points through which tests/test_compat_mappoint.py and tests/test_mappoint_batch_cpu.py
// build a small map, run the two MapPoint functions as single calls (map_model.cpp) or compat/MapPoint_batch.inl, and read the
// points back.  Keyframes are allocated one by one, so their addresses -- the order of std::map<KeyFrame*, size_t> -- need not
// follow their ids: mpt_obs reports the map's order.  Every entry point returns 0, or -1 after any C++ exception, whose text
// mpt_error() then returns.
#include <cstring>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>
#include "orbx.h"
#include "MapPoint.h"
namespace ORB_SLAM2 {
#include "MapPoint_batch.inl"
}

using namespace ORB_SLAM2;

namespace {
std::string g_error;
std::vector<std::unique_ptr<KeyFrame> > g_kfs;
std::vector<std::unique_ptr<MapPoint> > g_mps;

template <typename F> int Guard(F f) {
    try { f(); return 0; }
    catch (const std::exception &e) { g_error = e.what(); }
    catch (...) { g_error = "unknown exception"; }
    return -1;
}
}  // namespace

extern "C" {
const char *mpt_error() { return g_error.c_str(); }
int mpt_reset() { return Guard([&] { g_mps.clear(); g_kfs.clear(); }); }

// n keypoints: desc [n x 32], octave [n]; Ow = the camera centre
int mpt_add_keyframe(int n, const uint8_t *desc, const int *octave, const float *Ow, int levels, float factor, int *id) {
    return Guard([&] {
        std::unique_ptr<KeyFrame> k(new KeyFrame());
        k->mnId = g_kfs.size();
        k->mDescriptors = cv::Mat(n, 32, CV_8U);
        if (n) std::memcpy(k->mDescriptors.ptr<uint8_t>(), desc, (size_t)n * 32);
        k->mvKeysUn.resize((size_t)n);
        for (int i = 0; i < n; ++i) k->mvKeysUn[(size_t)i].octave = octave[i];
        k->mfScaleFactor = factor; k->mnScaleLevels = levels;
        k->mvScaleFactors.assign((size_t)levels, 1.0f);
        for (int l = 1; l < levels; ++l) k->mvScaleFactors[(size_t)l] = k->mvScaleFactors[(size_t)l - 1] * factor;
        k->Ow = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; ++c) k->Ow.at<float>(c) = Ow[c];
        *id = (int)g_kfs.size();
        g_kfs.push_back(std::move(k));
    });
}
int mpt_kf_set_bad(int kf) { return Guard([&] { g_kfs.at((size_t)kf)->mbBad = true; }); }

// a point with a given state (what a refresh must leave alone where it returns early)
int mpt_add_point(const float *pos, int ref_kf, const uint8_t *desc, const float *normal, float dmin, float dmax, int *id) {
    return Guard([&] {
        std::unique_ptr<MapPoint> p(new MapPoint());
        p->mWorldPos = cv::Mat(3, 1, CV_32F); p->mNormalVector = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; ++c) { p->mWorldPos.at<float>(c) = pos[c]; p->mNormalVector.at<float>(c) = normal[c]; }
        p->mDescriptor = cv::Mat(1, 32, CV_8U);
        std::memcpy(p->mDescriptor.ptr<uint8_t>(), desc, 32);
        p->mpRefKF = g_kfs.at((size_t)ref_kf).get();
        p->mfMinDistance = dmin; p->mfMaxDistance = dmax;
        *id = (int)g_mps.size();
        g_mps.push_back(std::move(p));
    });
}
// puts a point's refreshed members back (the same map, and so the same map order, is then refreshed the other way)
int mpt_restore(int mp, const uint8_t *desc, const float *normal, float dmin, float dmax) {
    return Guard([&] {
        MapPoint *p = g_mps.at((size_t)mp).get();
        p->mDescriptor = cv::Mat(1, 32, CV_8U);
        std::memcpy(p->mDescriptor.ptr<uint8_t>(), desc, 32);
        p->mNormalVector = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; ++c) p->mNormalVector.at<float>(c) = normal[c];
        p->mfMinDistance = dmin; p->mfMaxDistance = dmax;
    });
}
int mpt_observe(int mp, int kf, int idx) {
    return Guard([&] {
        KeyFrame *k = g_kfs.at((size_t)kf).get();
        k->mvKeysUn.at((size_t)idx);
        g_mps.at((size_t)mp)->mObservations[k] = (size_t)idx;
    });
}
int mpt_set_bad(int mp) { return Guard([&] { MapPoint *p = g_mps.at((size_t)mp).get(); p->mbBad = true; p->mObservations.clear(); }); }

// the observations in the map's order
int mpt_obs(int mp, int *kf, int *idx, int cap, int *n) {
    return Guard([&] {
        MapPoint *p = g_mps.at((size_t)mp).get();
        int e = 0;
        for (auto it = p->mObservations.begin(); it != p->mObservations.end(); ++it, ++e)
            if (e < cap) { kf[e] = (int)it->first->mnId; idx[e] = (int)it->second; }
        *n = e;
    });
}
// out = normal x, y, z, mfMinDistance, mfMaxDistance
int mpt_state(int mp, uint8_t *desc, float *out) {
    return Guard([&] {
        MapPoint *p = g_mps.at((size_t)mp).get();
        std::memcpy(desc, p->mDescriptor.ptr<uint8_t>(), 32);
        for (int c = 0; c < 3; ++c) out[c] = p->mNormalVector.at<float>(c);
        out[3] = p->mfMinDistance; out[4] = p->mfMaxDistance;
    });
}
// the loop of single calls over list[0 .. n): list entries < 0 stand for NULL and are skipped as a caller's loop skips them
int mpt_single_loop(const int *list, int n, int descriptors, int normal_and_depth) {
    return Guard([&] {
        for (int i = 0; i < n; ++i) {
            if (list[i] < 0) continue;
            MapPoint *p = g_mps.at((size_t)list[i]).get();
            if (descriptors) p->ComputeDistinctiveDescriptors();
            if (normal_and_depth) p->UpdateNormalAndDepth();
        }
    });
}
int mpt_refresh_batch(const int *list, int n, int descriptors, int normal_and_depth) {
    return Guard([&] {
        std::vector<MapPoint *> v;
        for (int i = 0; i < n; ++i) v.push_back(list[i] < 0 ? static_cast<MapPoint *>(NULL) : g_mps.at((size_t)list[i]).get());
        MapPoint::RefreshBatch(v, descriptors != 0, normal_and_depth != 0);
    });
}
}
