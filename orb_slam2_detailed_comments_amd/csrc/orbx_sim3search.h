// orbx_sim3search.h -- ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1433-1684) from the pose algebra on, restated once as scalar
// code shared by the host path (orbx_sim3search.cpp) and the kernels (k_sim3s_project, k_sim3s_cand, k_sim3s_mutual), and the
// layout of a batched call (orbx_search_by_sim3_batch).  tests/sim3_search_model.py restates it independently in numpy.
//
// Arithmetic: every expression in the reference's order; the cv::Mat operations follow the rule at the top of
// tests/compat_runtime/opencv2/core/core.hpp, which the compiled reference of oracle/ref/matcher/ is built against:
//   scalar * Mat      each element (float)((double)elem * scalar)
//   Mat * Mat         a double accumulator starting at 0.0 over k = 0, 1, 2, rounded once (the products of floats are exact in
//                     double, so a contracting compiler changes nothing)
//   Mat + Mat, -Mat   in float
//   cv::norm          (float)sqrt of the double sum of squares in element order
// The only expressions the reference's -mfma build contracts are u = fx * x + cx and v = fy * y + cy: fmaf under
// ORBX_FP_GCC_FMA, two roundings under ORBX_FP_STRICT.  Division and square root are the correctly rounded IEEE double
// operations on both sides; the library is built with -ffp-contract=off.  HIP-free: tests/san_sim3search.cpp builds the host
// half alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <math.h>
#include "orbx_ransac.h"   // ORBX_HD, orbx_canonf, orbx_pad256, include/orbx.h
#include "orbx_track.h"    // DTrackQ, ORBX_PS_LEVELS, orbx_predict_scale_level

enum { ORBX_SIM3S_TH_HIGH = 100, ORBX_SIM3S_GRID_COLS = 64, ORBX_SIM3S_GRID_ROWS = 48,
       ORBX_SIM3S_GRID_CELLS = ORBX_SIM3S_GRID_COLS * ORBX_SIM3S_GRID_ROWS };

// One direction of one problem: the source keyframe's pose [Rw | tw] and the similarity [sR | t] into the target's camera.
// Direction 0: KF1's points into KF2 (R1w, t1w, sR21, t21); direction 1: KF2's points into KF1 (R2w, t2w, sR12, t12).
struct OrbxSim3sDir { float Rw[9], tw[3], sR[9], t[3]; };
struct DSim3sProb {
    int32_t kf[2];                      // kf[0] = kf1, kf[1] = kf2: direction d projects kf[d]'s points into kf[1 - d]
    int32_t n[2];                       // their feature counts
    int32_t q_off;                      // first query: direction 0 at [q_off, q_off + n[0]), direction 1 behind it
    int32_t m_off;                      // first entry of matches12
    float th;
    int32_t pad;
    OrbxSim3sDir dir[2];
    int32_t pad2[8];
};
static_assert(sizeof(OrbxSim3sDir) == 96 && sizeof(DSim3sProb) == 256, "packed for the device");
// What the projection reads of a feature's MapPoint
struct DSim3sPt { float P[3], dmin, dmax; int32_t has; };
static_assert(sizeof(DSim3sPt) == 24, "packed for the device");
// The camera (KF1's intrinsics, as the reference reads them for both directions), the image bounds, and the handle's tables
struct OrbxSim3sCam {
    float fx, fy, cx, cy, minx, maxx, miny, maxy;
    int32_t fma_mode, nlevels;
    float thr[ORBX_PS_LEVELS], scale[ORBX_PS_LEVELS];
};
struct OrbxSim3sGrid { float minx, miny, winv, hinv; };   // DGrid of orbx_device.h for the HIP-free side

// one row of a matrix product with a 3-vector
ORBX_HD static inline float orbx_sim3s_dot3(const float *m, float x, float y, float z) {
    double s = 0.0;
    s += (double)m[0] * (double)x;
    s += (double)m[1] * (double)y;
    s += (double)m[2] * (double)z;
    return (float)s;
}
// sR12 = s12 * R12, sR21 = (1.0 / s12) * R12.t(), t21 = -sR21 * t12 (:1454-1456), once per problem
static inline void orbx_sim3s_similarity(float s12, const float *R12, const float *t12, float *sR12, float *sR21, float *t21) {
    const double s = (double)s12, inv = 1.0 / (double)s12;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            sR12[3 * r + c] = (float)((double)R12[3 * r + c] * s);
            sR21[3 * r + c] = (float)((double)R12[3 * c + r] * inv);
        }
    float neg[9];
    for (int i = 0; i < 9; ++i) neg[i] = -sR21[i];
    for (int r = 0; r < 3; ++r) t21[r] = orbx_sim3s_dot3(neg + 3 * r, t12[0], t12[1], t12[2]);
}

struct OrbxSim3sProj { int status; float u, v, r; int level; };
// Lines :1503-1541 / :1594-1625 for one MapPoint that is searched (good point, not already matched): the status
// (ORBX_SIM3S_BEHIND .. ORBX_SIM3S_DISTANCE, or ORBX_SIM3S_NO_CANDIDATE for "goes on to the search"), the projection where it
// was computed, the predicted level and the window radius where the point reached the search.
ORBX_HD static inline OrbxSim3sProj orbx_sim3s_project(const OrbxSim3sDir &D, const OrbxSim3sCam &C, float th, const DSim3sPt &T) {
    OrbxSim3sProj o;
    o.status = ORBX_SIM3S_BEHIND; o.u = 0.0f; o.v = 0.0f; o.r = -1.0f; o.level = -1;
    float a[3], c[3];
ORBX_UNROLL
    for (int i = 0; i < 3; ++i) a[i] = orbx_sim3s_dot3(D.Rw + 3 * i, T.P[0], T.P[1], T.P[2]) + D.tw[i];
ORBX_UNROLL
    for (int i = 0; i < 3; ++i) c[i] = orbx_sim3s_dot3(D.sR + 3 * i, a[0], a[1], a[2]) + D.t[i];
    if ((double)c[2] < 0.0) return o;
    const float invz = (float)(1.0 / (double)c[2]);
    const float x = c[0] * invz, y = c[1] * invz;
    float u, v;
    if (C.fma_mode) { u = __builtin_fmaf(C.fx, x, C.cx); v = __builtin_fmaf(C.fy, y, C.cy); }
    else { u = C.fx * x + C.cx; v = C.fy * y + C.cy; }
    o.u = orbx_canonf(u); o.v = orbx_canonf(v);
    o.status = ORBX_SIM3S_OUTSIDE;
    if (!(u >= C.minx && u < C.maxx && v >= C.miny && v < C.maxy)) return o;
    const float maxDistance = 1.2f * T.dmax, minDistance = 0.8f * T.dmin;
    double s2 = 0.0;
    s2 += (double)c[0] * (double)c[0];
    s2 += (double)c[1] * (double)c[1];
    s2 += (double)c[2] * (double)c[2];
    const float dist3D = (float)sqrt(s2);
    o.status = ORBX_SIM3S_DISTANCE;
    if (dist3D < minDistance || dist3D > maxDistance) return o;
    const float ratio = T.dmax / dist3D;
    int level = 0;
    float sc = C.scale[0];
ORBX_UNROLL
    for (int l = 1; l < ORBX_PS_LEVELS; ++l) {
        const bool up = l < C.nlevels && ratio >= C.thr[l];
        level += up ? 1 : 0;
    }
ORBX_UNROLL
    for (int l = 1; l < ORBX_PS_LEVELS; ++l) sc = level == l ? C.scale[l] : sc;   // selects: the table stays in registers
    o.level = level;
    o.r = th * sc;
    o.status = ORBX_SIM3S_NO_CANDIDATE;
    return o;
}
// the status and vnMatch entry of a searched point from the smallest key dist << 16 | visiting position (0xffffffff: none) and
// the feature that key belongs to
ORBX_HD static inline int orbx_sim3s_outcome(uint32_t key, int idx, int32_t *best) {
    *best = -1;
    if (key == 0xffffffffu) return ORBX_SIM3S_NO_CANDIDATE;
    if ((key >> 16) > (uint32_t)ORBX_SIM3S_TH_HIGH) return ORBX_SIM3S_TOO_FAR;
    *best = idx;
    return ORBX_SIM3S_MATCH;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Layout of one call.  The pool's keyframes are packed `fstride` records apart (fstride = the largest n).
// Uploaded block (one copy): counters (256 bytes, zero: [0] = live queries) | n per keyframe | problems | keypoints |
//   descriptors | MapPoint records | MapPoint descriptors | per query the "already matched" flag.
// Device only: bucket offsets | bucket items | queries (DTrackQ) | the compacted list of live queries.
// Downloaded block: nfound per problem | matches12 (ragged, problem order) | and for a debug call best | level | uv | status
//   per query (query order: problem, direction, feature).
struct OrbxSim3sPlan {
    int nkf = 0, nproblems = 0, fstride = 0, max_n = 0;
    size_t nq = 0, nm = 0;
    size_t o_ctr = 0, o_cnt = 0, o_prob = 0, o_keys = 0, o_desc = 0, o_pt = 0, o_pdesc = 0, o_flag = 0, in_bytes = 0;
    size_t o_cb = 0, o_it = 0, o_q = 0, o_live = 0, o_out = 0, dev_bytes = 0;
    size_t o_nf = 0, o_m = 0, out_small = 0, o_best = 0, o_level = 0, o_uv = 0, o_status = 0, out_bytes = 0;   // relative to o_out
};
struct DSim3sArgs {                     // what the kernels get, by value
    OrbxSim3sCam cam;
    const int32_t *cnt; const DSim3sProb *prob; const orbx_keypoint *keys; const uint8_t *desc; const DSim3sPt *pt;
    const uint8_t *pdesc; const uint8_t *flag;
    int32_t *ctr; int32_t *cb; uint16_t *items; DTrackQ *q; int32_t *live;
    int32_t *nfound; int32_t *matches; int32_t *best; int32_t *level; float *uv; uint8_t *status;
    int32_t nkf, nproblems, fstride, max_n, nq;
};
static inline DSim3sArgs orbx_sim3s_args(const OrbxSim3sPlan &p, const OrbxSim3sCam &cam, uint8_t *in, uint8_t *dev) {
    DSim3sArgs a;
    a.cam = cam;
    a.ctr = (int32_t *)(in + p.o_ctr); a.cnt = (const int32_t *)(in + p.o_cnt); a.prob = (const DSim3sProb *)(in + p.o_prob);
    a.keys = (const orbx_keypoint *)(in + p.o_keys); a.desc = in + p.o_desc; a.pt = (const DSim3sPt *)(in + p.o_pt);
    a.pdesc = in + p.o_pdesc; a.flag = in + p.o_flag;
    a.cb = (int32_t *)(dev + p.o_cb); a.items = (uint16_t *)(dev + p.o_it); a.q = (DTrackQ *)(dev + p.o_q);
    a.live = (int32_t *)(dev + p.o_live);
    uint8_t *out = dev + p.o_out;
    a.nfound = (int32_t *)(out + p.o_nf); a.matches = (int32_t *)(out + p.o_m); a.best = (int32_t *)(out + p.o_best);
    a.level = (int32_t *)(out + p.o_level); a.uv = (float *)(out + p.o_uv); a.status = out + p.o_status;
    a.nkf = p.nkf; a.nproblems = p.nproblems; a.fstride = p.fstride; a.max_n = p.max_n; a.nq = (int32_t)p.nq;
    return a;
}

// Validation of the whole call, before any device work, and the layout.  *why names the offending argument.
orbx_status orbx_sim3s_plan(int nkeyframes, const orbx_sim3_search_keyframe *keyframes, int nproblems,
                            const orbx_sim3_search_problem *problems, const float *camera4, const float *bounds4, int nlevels,
                            int32_t *const *matches12, const int *nfound, OrbxSim3sPlan &plan, const char **why);
void orbx_sim3s_camera(const float *camera4, const float *bounds4, int fma_mode, int nlevels, const float *thr, const float *scale,
                       OrbxSim3sCam &cam, OrbxSim3sGrid &grid);
// Packing into `dst` (plan.in_bytes bytes).  The caller's arrays are not read afterwards.
void orbx_sim3s_pack(const orbx_sim3_search_keyframe *keyframes, const orbx_sim3_search_problem *problems, const OrbxSim3sPlan &plan,
                     uint8_t *dst);
// The host path over the packed block: Frame grid, projection, the reference's bucket walk, the mutual test; writes the
// downloaded block's layout (all of it) into out (plan.out_bytes bytes).
void orbx_sim3s_host_run(const OrbxSim3sPlan &plan, const OrbxSim3sCam &cam, const OrbxSim3sGrid &grid, const uint8_t *in, uint8_t *out);
// Scatter of the downloaded block into the caller's rows; dbg may be NULL
void orbx_sim3s_unpack(const OrbxSim3sPlan &plan, const uint8_t *in, const uint8_t *out,
                       int32_t *const *matches12, int *nfound, const orbx_sim3_search_debug *dbg);
