// tests/compat_essgraph/harness.cpp -- compat/Optimizer_essentialgraph.inl inside the function it belongs to, over the stand-ins
// of this directory, behind a C interface for tests/test_compat_essgraph.py (ctypes).
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <vector>
#include "orbx.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "Map.h"

namespace g2o {
// what the fragment reads of g2o::Sim3: rotation() with x(), y(), z(), w(); translation()[k]; scale()
struct Quat {
    double q[4];
    double x() const { return q[0]; }
    double y() const { return q[1]; }
    double z() const { return q[2]; }
    double w() const { return q[3]; }
};
struct Vec3 {
    double v[3];
    double operator[](int k) const { return v[k]; }
};
struct Sim3 {
    Quat r; Vec3 t; double s;
    const Quat &rotation() const { return r; }
    const Vec3 &translation() const { return t; }
    const double &scale() const { return s; }
};
}  // namespace g2o

namespace ORB_SLAM2 {
using namespace std;
std::vector<MapPoint *> MapPoint::refreshed;
int MapPoint::refreshFlags = 0;
struct LoopClosing {
    typedef map<KeyFrame *, g2o::Sim3> KeyFrameAndPose;
};

static void OptimizeEssentialGraph(Map *pMap, KeyFrame *pLoopKF, KeyFrame *pCurKF, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                   const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                   const map<KeyFrame *, set<KeyFrame *> > &LoopConnections, const bool &bFixScale) {
    const vector<KeyFrame *> vpKFs = pMap->GetAllKeyFrames();
    const vector<MapPoint *> vpMPs = pMap->GetAllMapPoints();
    const unsigned int nMaxKFid = pMap->GetMaxKFid();
    const int minFeat = 100;
#include "Optimizer_essentialgraph.inl"
}
}  // namespace ORB_SLAM2

using namespace ORB_SLAM2;

static g2o::Sim3 sim3_of(const double *s) {
    g2o::Sim3 S;
    for (int k = 0; k < 4; ++k) S.r.q[k] = s[k];
    for (int k = 0; k < 3; ++k) S.t.v[k] = s[4 + k];
    S.s = s[7];
    return S;
}

// One map from flat arrays.  Keyframe k has mnId k.  weights [n][n] (0: not connected); parents [n] (-1: none); loop_edges and
// loop_conns are (i, j) pairs (loop_edges both ways as the caller lists them); corrected / non_corrected [n][8] with their
// flags.  Points: world [np][3], ref_kf [np], bad [np], corrected_by_cur [np] with corrected_ref [np].
// Returns 0, or -1 when the fragment threw; Tcw_out [n][16] (every keyframe's pose afterwards), world_out [np][3], info[0] =
// SetPose calls, info[1] = SetWorldPos calls, info[2] = points handed to RefreshBatch, info[3] = its flags.
extern "C" int eg_compat_run(int n, const float *Tcw, const uint8_t *bad, const int32_t *parents, const int32_t *weights, int nloop,
                             const int32_t *loop_edges, int nconn, const int32_t *loop_conns, const uint8_t *has_corrected,
                             const double *corrected, const uint8_t *has_non_corrected, const double *non_corrected, int cur, int loop,
                             int fix_scale, int np, const float *world, const int32_t *ref_kf, const uint8_t *pt_bad,
                             const uint8_t *corrected_by_cur, const int32_t *corrected_ref, float *Tcw_out, float *world_out,
                             int32_t *info) {
    std::vector<KeyFrame> kfs((size_t)n);
    std::vector<MapPoint> pts((size_t)np);
    Map map;
    for (int k = 0; k < n; ++k) {
        KeyFrame &K = kfs[(size_t)k];
        K.mnId = (unsigned long)k;
        K.mbBad = bad[k] != 0;
        K.Tcw = cv::Mat(4, 4, CV_32F);
        std::memcpy(K.Tcw.ptr<float>(), Tcw + 16 * (size_t)k, 16 * sizeof(float));
        if (parents[k] >= 0) { K.mpParent = &kfs[(size_t)parents[k]]; kfs[(size_t)parents[k]].mspChildrens.insert(&K); }
        for (int j = 0; j < n; ++j) if (weights[(size_t)k * n + j] > 0) K.mConnectedKeyFrameWeights[&kfs[(size_t)j]] = weights[(size_t)k * n + j];
        map.mvpKeyFrames.push_back(&K);
    }
    map.mnMaxKFid = n > 0 ? (unsigned long)(n - 1) : 0;
    for (int e = 0; e < nloop; ++e) kfs[(size_t)loop_edges[2 * e]].mspLoopEdges.insert(&kfs[(size_t)loop_edges[2 * e + 1]]);
    std::map<KeyFrame *, std::set<KeyFrame *> > conns;
    for (int e = 0; e < nconn; ++e) conns[&kfs[(size_t)loop_conns[2 * e]]].insert(&kfs[(size_t)loop_conns[2 * e + 1]]);
    LoopClosing::KeyFrameAndPose Corrected, NonCorrected;
    for (int k = 0; k < n; ++k) {
        if (has_corrected[k]) Corrected[&kfs[(size_t)k]] = sim3_of(corrected + 8 * (size_t)k);
        if (has_non_corrected[k]) NonCorrected[&kfs[(size_t)k]] = sim3_of(non_corrected + 8 * (size_t)k);
    }
    for (int p = 0; p < np; ++p) {
        MapPoint &M = pts[(size_t)p];
        M.mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; ++c) M.mWorldPos.at<float>(c) = world[3 * (size_t)p + c];
        M.mbBad = pt_bad[p] != 0;
        M.mpRefKF = &kfs[(size_t)ref_kf[p]];
        M.mnCorrectedByKF = corrected_by_cur[p] ? (unsigned long)cur : (unsigned long)n + 7;
        M.mnCorrectedReference = (unsigned long)corrected_ref[p];
        map.mvpMapPoints.push_back(&M);
    }
    MapPoint::refreshed.clear(); MapPoint::refreshFlags = 0;
    const bool bFixScale = fix_scale != 0;
    try {
        OptimizeEssentialGraph(&map, &kfs[(size_t)loop], &kfs[(size_t)cur], NonCorrected, Corrected, conns, bFixScale);
    } catch (const std::exception &) {
        return -1;
    }
    int nset = 0, nworld = 0;
    for (int k = 0; k < n; ++k) {
        nset += kfs[(size_t)k].nSetPose;
        std::memcpy(Tcw_out + 16 * (size_t)k, kfs[(size_t)k].Tcw.ptr<float>(), 16 * sizeof(float));
    }
    for (int p = 0; p < np; ++p) {
        nworld += pts[(size_t)p].nSetWorldPos;
        for (int c = 0; c < 3; ++c) world_out[3 * (size_t)p + c] = pts[(size_t)p].mWorldPos.at<float>(c);
    }
    info[0] = nset; info[1] = nworld; info[2] = (int32_t)MapPoint::refreshed.size(); info[3] = MapPoint::refreshFlags;
    return 0;
}
