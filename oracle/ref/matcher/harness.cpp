// oracle/ref/matcher: the extern "C" entry points of tests/compat_runtime/harness.cpp (same names, same arguments) over the
// REFERENCE's own ORBmatcher and MapPoint, compiled unmodified from src/ORBmatcher.cc and src/MapPoint.cc (build_ref.py names
// the sources and flags).  Frame, KeyFrame and Map are the stand-ins of this directory; cv::Mat is the one of
// tests/compat_runtime/.  Nothing here restates what the matcher or MapPoint compute: the functions move data in and out.
// The batched entry points run the plain loop of single reference calls.  The extractor, stereo and undistort entry points do
// not exist here.  Every entry point returns 0, or -1 after any C++ exception, whose text h_error() then returns.
//
// MapPoint keys its observations by KeyFrame pointer, so their order is the order of the keyframes' addresses.  The keyframes
// of a scene live in one array reserved up front: address order is id order, the order tests/compat_runtime/MapPoint.h uses.
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "ORBmatcher.h"

using namespace ORB_SLAM2;

namespace ORB_SLAM2 {
float Frame::mnMinX = 0.f, Frame::mnMaxX = 0.f, Frame::mnMinY = 0.f, Frame::mnMaxY = 0.f;
std::set<MapPoint *> KeyFrame::GetMapPoints() {
    std::set<MapPoint *> s;
    for (size_t i = 0; i < mvpMapPoints.size(); ++i)
        if (mvpMapPoints[i] && !mvpMapPoints[i]->isBad()) s.insert(mvpMapPoints[i]);
    return s;
}
}  // namespace ORB_SLAM2

namespace {
const size_t kMaxKeyFrames = 4096;
std::string g_error;
Map g_map;
// the constructor MapPoint(Pos, pRefKF, pMap) leaves normal, descriptor and distances empty; a scene sets them directly
struct Point : public MapPoint {
    Point(const cv::Mat &pos, KeyFrame *ref, const cv::Mat &normal, const cv::Mat &desc, float minDist, float maxDist)
        : MapPoint(pos, ref, &g_map) {
        mNormalVector = normal.clone(); mDescriptor = desc.clone(); mfMinDistance = minDist; mfMaxDistance = maxDist;
    }
};
std::vector<std::unique_ptr<Point> > g_mps;
std::vector<KeyFrame> g_kfs;
std::vector<std::unique_ptr<Frame> > g_frames;
KeyFrame g_origin(0, 0, 1, 1.2f);     // reference keyframe of every point (only its ids are read)

template <typename F> int Guard(F f) {
    try { f(); return 0; }
    catch (const std::exception &e) { g_error = e.what(); }
    catch (const std::string &e) { g_error = e; }
    catch (...) { g_error = "unknown exception"; }
    return -1;
}
MapPoint *MP(int i) { return i < 0 ? static_cast<MapPoint *>(NULL) : g_mps.at((size_t)i).get(); }
int Id(const MapPoint *p) { return p ? (int)p->mnId : -1; }
KeyFrame *KF(int i) { return &g_kfs.at((size_t)i); }
Frame *FR(int i) { return g_frames.at((size_t)i).get(); }
std::vector<MapPoint *> MPs(const int *ids, int n) {
    std::vector<MapPoint *> v((size_t)n);
    for (int i = 0; i < n; ++i) v[i] = MP(ids[i]);
    return v;
}
std::vector<cv::KeyPoint> Keys(const void *k, int n) {
    const cv::KeyPoint *p = static_cast<const cv::KeyPoint *>(k);
    return std::vector<cv::KeyPoint>(p, p + n);
}
cv::Mat Desc(const uint8_t *d, int n) {
    cv::Mat m(n, 32, CV_8U);
    if (n) std::memcpy(m.data, d, (size_t)n * 32);
    return m;
}
cv::Mat Floats(const float *v, int r, int c) {
    cv::Mat m(r, c, CV_32F);
    for (int i = 0; i < r; ++i) for (int j = 0; j < c; ++j) m.at<float>(i, j) = v[c * i + j];
    return m;
}
DBoW2::FeatureVector FeatVec(int nnodes, const uint32_t *node, const int32_t *begin, const uint32_t *index) {
    DBoW2::FeatureVector fv;
    for (int i = 0; i < nnodes; ++i) fv[node[i]] = std::vector<unsigned int>(index + begin[i], index + begin[i + 1]);
    return fv;
}
void Put(const std::vector<MapPoint *> &v, int *out) { for (size_t i = 0; i < v.size(); ++i) out[i] = Id(v[i]); }
MapPoint *NewPoint(const cv::Mat &pos, const cv::Mat &normal, const cv::Mat &desc, float minDist, float maxDist) {
    g_mps.emplace_back(new Point(pos, &g_origin, normal, desc, minDist, maxDist));
    if (g_mps.back()->mnId + 1 != g_mps.size()) throw std::runtime_error("MapPoint ids out of step with the scene");
    return g_mps.back().get();
}
}  // namespace

extern "C" {

const char *h_error() { return g_error.c_str(); }
const char *h_compiler() { return __VERSION__; }
// 1 when the compiler was allowed to contract a * b + c (the -mfma build), 0 otherwise
int h_fp_fast_fma() {
#ifdef __FMA__
    return 1;
#else
    return 0;
#endif
}

int h_reset() {
    return Guard([&] {
        g_mps.clear(); g_kfs.clear(); g_frames.clear();
        g_kfs.reserve(kMaxKeyFrames);
        MapPoint::nNextId = 0;
    });
}

int h_set_frame_bounds(float minx, float maxx, float miny, float maxy) {
    return Guard([&] { Frame::mnMinX = minx; Frame::mnMaxX = maxx; Frame::mnMinY = miny; Frame::mnMaxY = maxy; });
}

// ---- the map

// K = (fx, fy, cx, cy); bounds = (minx, maxx, miny, maxy); Tcw row-major 4x4
int h_add_keyframe(int n, const void *keys, const uint8_t *desc, const float *u_right, const float *Tcw, const float *K, float mbf,
                   const int *bounds, int levels, float scale_factor, int nnodes, const uint32_t *node, const int32_t *begin,
                   const uint32_t *index, int *id) {
    return Guard([&] {
        if (g_kfs.capacity() < kMaxKeyFrames) g_kfs.reserve(kMaxKeyFrames);
        if (g_kfs.size() == kMaxKeyFrames) throw std::runtime_error("too many keyframes for one scene");
        g_kfs.emplace_back(g_kfs.size(), n, levels, scale_factor);
        KeyFrame *k = &g_kfs.back();
        k->mvKeys = k->mvKeysUn = Keys(keys, n);
        k->mDescriptors = Desc(desc, n);
        k->mvuRight.assign(u_right, u_right + n);
        k->mvDepth.assign((size_t)n, -1.f);
        k->SetPose(Floats(Tcw, 4, 4));
        k->fx = K[0]; k->fy = K[1]; k->cx = K[2]; k->cy = K[3]; k->invfx = 1.f / K[0]; k->invfy = 1.f / K[1];
        k->mbf = mbf; k->mb = mbf / K[0];
        k->mnMinX = bounds[0]; k->mnMaxX = bounds[1]; k->mnMinY = bounds[2]; k->mnMaxY = bounds[3];
        k->mFeatVec = FeatVec(nnodes, node, begin, index);
        *id = (int)g_kfs.size() - 1;
    });
}

// keys / keys_un: N keypoints each; Tcw may be NULL (no pose)
int h_add_frame(int n, const void *keys, const void *keys_un, const uint8_t *desc, const float *u_right, const float *Tcw,
                const float *K, float mb, float mbf, int levels, float scale_factor, int nnodes, const uint32_t *node,
                const int32_t *begin, const uint32_t *index, int *id) {
    return Guard([&] {
        std::unique_ptr<Frame> f(new Frame());
        f->mnId = g_frames.size();
        f->N = n;
        f->mvKeys = Keys(keys, n); f->mvKeysUn = Keys(keys_un, n);
        f->mDescriptors = Desc(desc, n);
        f->mvuRight.assign(u_right, u_right + n);
        f->mvDepth.assign((size_t)n, -1.f);
        f->mvpMapPoints.assign((size_t)n, static_cast<MapPoint *>(NULL));
        f->mvbOutlier.assign((size_t)n, false);
        if (Tcw) f->mTcw = Floats(Tcw, 4, 4);
        f->fx = K[0]; f->fy = K[1]; f->cx = K[2]; f->cy = K[3]; f->invfx = 1.f / K[0]; f->invfy = 1.f / K[1];
        f->mb = mb; f->mbf = mbf;
        f->mnScaleLevels = levels; f->mfScaleFactor = scale_factor; f->mfLogScaleFactor = std::log(scale_factor);
        KeyFrame::ScaleTables(levels, scale_factor, f->mvScaleFactors, f->mvLevelSigma2, f->mvInvLevelSigma2);
        f->mvInvScaleFactors.resize(f->mvScaleFactors.size());
        for (size_t l = 0; l < f->mvScaleFactors.size(); ++l) f->mvInvScaleFactors[l] = 1.f / f->mvScaleFactors[l];
        f->mFeatVec = FeatVec(nnodes, node, begin, index);
        *id = (int)g_frames.size();
        g_frames.push_back(std::move(f));
    });
}

int h_frame_set(int f, int idx, int mp, int outlier) {
    return Guard([&] { FR(f)->mvpMapPoints.at((size_t)idx) = MP(mp); FR(f)->mvbOutlier.at((size_t)idx) = outlier != 0; });
}

int h_add_mappoint(const float *pos, const float *normal, const uint8_t *desc, float min_dist, float max_dist, int *id) {
    return Guard([&] { *id = Id(NewPoint(Floats(pos, 3, 1), Floats(normal, 3, 1), Desc(desc, 1), min_dist, max_dist)); });
}

int h_mp_track(int mp, int in_view, float x, float y, float xr, int level, float view_cos) {
    return Guard([&] {
        MapPoint *p = MP(mp);
        p->mbTrackInView = in_view != 0; p->mTrackProjX = x; p->mTrackProjY = y; p->mTrackProjXR = xr;
        p->mnTrackScaleLevel = level; p->mTrackViewCos = view_cos;
    });
}

// keyframe kf observes point mp in slot idx (MapPoint::AddObservation + KeyFrame::AddMapPoint, as map building does)
int h_observe(int mp, int kf, int idx) {
    return Guard([&] {
        if (!MP(mp)) throw std::out_of_range("no such map point");
        KF(kf)->mvuRight.at((size_t)idx);                            // AddObservation reads it unchecked
        MP(mp)->AddObservation(KF(kf), (size_t)idx); KF(kf)->AddMapPoint(MP(mp), (size_t)idx);
    });
}
int h_set_bad(int mp) { return Guard([&] { g_mps.at((size_t)mp)->SetBadFlag(); }); }
int h_replace(int mp, int by) { return Guard([&] { g_mps.at((size_t)mp)->Replace(g_mps.at((size_t)by).get()); }); }
int h_compute_descriptor(int mp) { return Guard([&] { g_mps.at((size_t)mp)->ComputeDistinctiveDescriptors(); }); }

// bad flag, Observations(), descriptor and up to cap (keyframe, slot) observations in keyframe order
int h_mp_state(int mp, int *bad, int *nobs, uint8_t *desc, int *obs_kf, int *obs_idx, int cap, int *nentries) {
    return Guard([&] {
        MapPoint *p = g_mps.at((size_t)mp).get();
        *bad = p->isBad(); *nobs = p->Observations();
        const cv::Mat d = p->GetDescriptor();
        std::memcpy(desc, d.data, 32);
        const std::map<KeyFrame *, size_t> obs = p->GetObservations();
        int e = 0;
        for (auto it = obs.begin(); it != obs.end(); ++it, ++e)
            if (e < cap) { obs_kf[e] = (int)it->first->mnId; obs_idx[e] = (int)it->second; }
        *nentries = e;
    });
}
int h_kf_slots(int kf, int *out) { return Guard([&] { Put(KF(kf)->GetMapPointMatches(), out); }); }
int h_frame_slots(int f, int *out) { return Guard([&] { Put(FR(f)->mvpMapPoints, out); }); }
int h_predict_scale(int mp, float dist, int target, int is_frame, int *out) {
    return Guard([&] { *out = is_frame ? MP(mp)->PredictScale(dist, FR(target)) : MP(mp)->PredictScale(dist, KF(target)); });
}
int h_mp_invariance(int mp, float *lo, float *hi) {
    return Guard([&] { *lo = MP(mp)->GetMinDistanceInvariance(); *hi = MP(mp)->GetMaxDistanceInvariance(); });
}

// ---- the reference matcher (a matched MapPoint is reported by index, -1 = NULL)

int h_descriptor_distance(const uint8_t *a, const uint8_t *b, int *out) {
    return Guard([&] {
        const cv::Mat A = Desc(a, 2), B = Desc(b, 1);               // a second row of A: row(1) is a view with an offset
        *out = ORBmatcher::DescriptorDistance(A.row(1), B);
    });
}

int h_search_by_projection_mappoints(int f, const int *mps, int n, float th, float ratio, int *count) {
    return Guard([&] { ORBmatcher m(ratio, true); *count = m.SearchByProjection(*FR(f), MPs(mps, n), th); });
}

int h_search_by_projection_frame(int cur, int last, float th, int mono, int ori, int *count) {
    return Guard([&] { ORBmatcher m(0.9f, ori != 0); *count = m.SearchByProjection(*FR(cur), *FR(last), th, mono != 0); });
}

int h_search_by_projection_keyframe(int f, int kf, const int *found, int nfound, float th, int orbdist, int ori, int *count) {
    return Guard([&] {
        ORBmatcher m(0.9f, ori != 0);
        const std::vector<MapPoint *> v = MPs(found, nfound);
        const std::set<MapPoint *> s(v.begin(), v.end());
        *count = m.SearchByProjection(*FR(f), KF(kf), s, th, orbdist);
    });
}

// matched: in / out, one entry per slot of kf
int h_search_by_projection_sim3(int kf, const float *Scw, const int *pts, int npts, int *matched, int th, int *count) {
    return Guard([&] {
        ORBmatcher m(0.9f, true);
        std::vector<MapPoint *> vm = MPs(matched, KF(kf)->N);
        *count = m.SearchByProjection(KF(kf), Floats(Scw, 4, 4), MPs(pts, npts), vm, th);
        Put(vm, matched);
    });
}

int h_search_by_bow_frame(int kf, int f, float ratio, int ori, int *out, int *count) {
    return Guard([&] {
        ORBmatcher m(ratio, ori != 0);
        std::vector<MapPoint *> v;
        *count = m.SearchByBoW(KF(kf), *FR(f), v);
        Put(v, out);
    });
}

int h_search_by_bow_keyframes(int kf1, int kf2, float ratio, int ori, int *out, int *count) {
    return Guard([&] {
        ORBmatcher m(ratio, ori != 0);
        std::vector<MapPoint *> v;
        *count = m.SearchByBoW(KF(kf1), KF(kf2), v);
        Put(v, out);
    });
}

// out: K rows of N entries (N = the frame's / kf1's features); always the loop of single calls, whatever `batch` says
int h_search_by_bow_frame_batch(const int *kfs, int K, int f, float ratio, int ori, int batch, int *out, int *counts) {
    return Guard([&] {
        ORBmatcher m(ratio, ori != 0);
        std::vector<KeyFrame *> v((size_t)K);
        for (int k = 0; k < K; ++k) v[k] = KF(kfs[k]);
        std::vector<std::vector<MapPoint *> > vv;
        std::vector<int> n;
        (void)batch;
        vv.resize((size_t)K);
        for (int k = 0; k < K; ++k) n.push_back(m.SearchByBoW(v[k], *FR(f), vv[k]));
        if ((int)n.size() != K || (int)vv.size() != K) throw std::runtime_error("wrong number of results");
        for (int k = 0; k < K; ++k) { counts[k] = n[k]; Put(vv[k], out + (size_t)k * FR(f)->N); }
    });
}
int h_search_by_bow_keyframes_batch(int kf1, const int *kfs, int K, float ratio, int ori, int batch, int *out, int *counts) {
    return Guard([&] {
        ORBmatcher m(ratio, ori != 0);
        std::vector<KeyFrame *> v((size_t)K);
        for (int k = 0; k < K; ++k) v[k] = KF(kfs[k]);
        std::vector<std::vector<MapPoint *> > vv;
        std::vector<int> n;
        (void)batch;
        vv.resize((size_t)K);
        for (int k = 0; k < K; ++k) n.push_back(m.SearchByBoW(KF(kf1), v[k], vv[k]));
        if ((int)n.size() != K || (int)vv.size() != K) throw std::runtime_error("wrong number of results");
        for (int k = 0; k < K; ++k) { counts[k] = n[k]; Put(vv[k], out + (size_t)k * KF(kf1)->N); }
    });
}

// prev: 2 floats per F1 feature, in / out
int h_search_for_initialization(int f1, int f2, float *prev, int window, float ratio, int ori, int *m12, int *count) {
    return Guard([&] {
        ORBmatcher m(ratio, ori != 0);
        const int n1 = FR(f1)->N;
        std::vector<cv::Point2f> p((size_t)n1);
        for (int i = 0; i < n1; ++i) p[i] = cv::Point2f(prev[2 * i], prev[2 * i + 1]);
        std::vector<int> v;
        *count = m.SearchForInitialization(*FR(f1), *FR(f2), p, v, window);
        if ((int)v.size() != (int)FR(f1)->mvKeysUn.size()) throw std::runtime_error("vnMatches12 has the wrong size");
        for (int i = 0; i < n1; ++i) { m12[i] = v[i]; prev[2 * i] = p[i].x; prev[2 * i + 1] = p[i].y; }
    });
}

// pairs: 2 * cap entries (index in kf1, index in kf2)
int h_search_for_triangulation(int kf1, int kf2, const float *F12, int only_stereo, int ori, int *pairs, int cap, int *count) {
    return Guard([&] {
        ORBmatcher m(0.6f, ori != 0);
        std::vector<std::pair<size_t, size_t> > v;
        *count = m.SearchForTriangulation(KF(kf1), KF(kf2), Floats(F12, 3, 3), v, only_stereo != 0);
        if ((int)v.size() != *count || *count > cap) throw std::runtime_error("pair list does not match the count");
        for (size_t i = 0; i < v.size(); ++i) { pairs[2 * i] = (int)v[i].first; pairs[2 * i + 1] = (int)v[i].second; }
    });
}

// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:349-430) reduced to its map updates: neighbour k is searched (the single
// call; `batch` is accepted and ignored: the reference has no batched form) with F12s[9k..], then every `stride`-th returned pair becomes a new map
// point observed by kf1 and the neighbour, descriptor from kf1, before neighbour k+1 is searched.  pairs: K rows of 2 * cap.
int h_triangulation_loop(int kf1, const int *kfs, int K, const float *F12s, int only_stereo, int ori, int batch, int stride,
                         int *pairs, int cap, int *counts) {
    return Guard([&] {
        ORBmatcher m(0.6f, ori != 0);
        std::vector<KeyFrame *> v((size_t)K);
        for (int k = 0; k < K; ++k) v[k] = KF(kfs[k]);
        (void)batch;
        KeyFrame *k1 = KF(kf1);
        for (int k = 0; k < K; ++k) {
            std::vector<std::pair<size_t, size_t> > pr;
            const cv::Mat F = Floats(F12s + 9 * k, 3, 3);
            counts[k] = m.SearchForTriangulation(k1, v[k], F, pr, only_stereo != 0);
            if ((int)pr.size() != counts[k] || counts[k] > cap) throw std::runtime_error("pair list does not match the count");
            for (size_t i = 0; i < pr.size(); ++i) {
                pairs[(size_t)k * 2 * cap + 2 * i] = (int)pr[i].first; pairs[(size_t)k * 2 * cap + 2 * i + 1] = (int)pr[i].second;
                if (i % (size_t)stride) continue;
                const float pos[3] = {0.f, 0.f, 1.f}, nrm[3] = {0.f, 0.f, 1.f};
                MapPoint *p = NewPoint(Floats(pos, 3, 1), Floats(nrm, 3, 1), k1->mDescriptors.row((int)pr[i].first), 1.f, 2.f);
                p->AddObservation(k1, pr[i].first); p->AddObservation(v[k], pr[i].second);
                k1->AddMapPoint(p, pr[i].first); v[k]->AddMapPoint(p, pr[i].second);
                p->ComputeDistinctiveDescriptors();
            }
        }
    });
}

// matches: in / out, one entry per slot of kf1; R12 row-major 3x3
int h_search_by_sim3(int kf1, int kf2, int *matches, float s12, const float *R12, const float *t12, float th, int *count) {
    return Guard([&] {
        ORBmatcher m(0.75f, true);
        std::vector<MapPoint *> v = MPs(matches, KF(kf1)->N);
        *count = m.SearchBySim3(KF(kf1), KF(kf2), v, s12, Floats(R12, 3, 3), Floats(t12, 3, 1), th);
        Put(v, matches);
    });
}

int h_fuse(int kf, const int *mps, int n, float th, int *count) {
    return Guard([&] { ORBmatcher m(0.6f, true); *count = m.Fuse(KF(kf), MPs(mps, n), th); });
}

// mode 0 and 1: for k: Fuse(kf_k, list) (the loop FuseBatch claims to equal); 2: for k: for i: Fuse(kf_k, {p_i})
int h_fuse_loop(const int *kfs, int K, const int *mps, int n, float th, int mode, int *count) {
    return Guard([&] {
        ORBmatcher m(0.6f, true);
        std::vector<KeyFrame *> v((size_t)K);
        for (int k = 0; k < K; ++k) v[k] = KF(kfs[k]);
        const std::vector<MapPoint *> list = MPs(mps, n);
        int total = 0;
        for (int k = 0; k < K; ++k) {
            if (mode != 2) total += m.Fuse(v[k], list, th);
            else for (int i = 0; i < n; ++i) total += m.Fuse(v[k], std::vector<MapPoint *>(1, list[i]), th);
        }
        *count = total;
    });
}

// replace: out, one entry per point (-1 = NULL)
int h_fuse_sim3(int kf, const float *Scw, const int *mps, int n, float th, int *replace, int *count) {
    return Guard([&] {
        ORBmatcher m(0.6f, true);
        std::vector<MapPoint *> rep((size_t)n, static_cast<MapPoint *>(NULL));
        *count = m.Fuse(KF(kf), Floats(Scw, 4, 4), MPs(mps, n), th, rep);
        Put(rep, replace);
    });
}

}  // extern "C"
