// orbx_track_pack.cpp -- host side of the batched tracking matchers (orbx_track.h): validation of a call and the packing of all
// its problems' host arrays into one staging block.  HIP-free: tests/san_track_pack.cpp builds it alone under the sanitizers.
// Built with -ffp-contract=off like the rest of the library: the pose products below round as the single calls' do.
#include <cmath>
#include <cstring>
#include <limits>
#include "orbx_track.h"

static inline size_t tp_pad256(size_t b) { return (b + 255) & ~(size_t)255; }

static orbx_status tp_common(int nproblems, const void *problems, const OrbxTrackBatchArgs &a, const char **why) {
    if (nproblems < 0) { *why = "nproblems < 0"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !problems) { *why = "null problem array"; return ORBX_BAD_ARGUMENT; }
    if (a.cap <= 0) { *why = "cap <= 0"; return ORBX_BAD_ARGUMENT; }
    if (a.nframes <= 0 && nproblems > 0) { *why = "nframes <= 0"; return ORBX_BAD_ARGUMENT; }
    if (a.cap > 65535) { *why = "cap > 65535 (bucket entries are 16-bit feature indices)"; return ORBX_UNSUPPORTED; }
    if (!a.device_pointers_ok) { *why = "null device buffer"; return ORBX_BAD_ARGUMENT; }
    return ORBX_OK;
}

static orbx_status tp_layout(OrbxTrackPlan &p, const char **why) {
    if (p.nq > (size_t)0x7fffffff / 64) { *why = "too many points for 32-bit offsets"; return ORBX_UNSUPPORTED; }
    p.o_prob = 0;
    p.o_q = tp_pad256((size_t)p.nproblems * sizeof(DTrackProb));
    p.o_desc = p.o_q + tp_pad256(p.nq * sizeof(DTrackQ));
    p.o_seed = p.o_desc + tp_pad256(p.nq * 32);
    p.in_bytes = p.o_seed + tp_pad256((size_t)p.nproblems * p.seed_words * sizeof(uint32_t));
    p.o_cand = p.in_bytes;
    p.o_ev = p.o_cand + tp_pad256(p.nq * 16);
    p.dev_bytes = p.o_ev + tp_pad256(p.nq * sizeof(int32_t));
    return ORBX_OK;
}

orbx_status orbx_track_frame_plan(int nproblems, const orbx_track_frame_problem *problems, const OrbxTrackBatchArgs &a,
                                  OrbxTrackPlan &plan, const char **why) {
    plan = OrbxTrackPlan();
    const orbx_status st = tp_common(nproblems, problems, a, why);
    if (st != ORBX_OK) return st;
    plan.nproblems = nproblems;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_track_frame_problem &P = problems[k];
        if (P.frame < 0 || P.frame >= a.nframes) { *why = "frame outside [0, nframes)"; return ORBX_BAD_ARGUMENT; }
        const orbx_last_frame_view &L = P.last;
        if (L.n < 0) { *why = "last.n < 0"; return ORBX_BAD_ARGUMENT; }
        if (L.n > 0 && (!L.keys_un || !L.has_map_point || !L.world_pos || !L.mp_desc || !L.observations)) {
            *why = "null field of a last-frame view";
            return ORBX_BAD_ARGUMENT;
        }
        for (int i = 0; i < L.n; ++i)
            if (L.has_map_point[i] && (L.keys_un[i].octave < 0 || L.keys_un[i].octave >= a.nlevels)) {
                *why = "octave outside [0, nlevels) on a point with a MapPoint";
                return ORBX_BAD_ARGUMENT;
            }
        plan.nq += (size_t)L.n;
    }
    return tp_layout(plan, why);
}

orbx_status orbx_track_points_plan(int nproblems, const orbx_track_points_problem *problems, const OrbxTrackBatchArgs &a,
                                   OrbxTrackPlan &plan, const char **why) {
    plan = OrbxTrackPlan();
    const orbx_status st = tp_common(nproblems, problems, a, why);
    if (st != ORBX_OK) return st;
    plan.nproblems = nproblems;
    plan.seed_words = (a.cap + 31) / 32;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_track_points_problem &P = problems[k];
        if (P.frame < 0 || P.frame >= a.nframes) { *why = "frame outside [0, nframes)"; return ORBX_BAD_ARGUMENT; }
        const orbx_mappoint_view &M = P.points;
        if (M.n < 0) { *why = "points.n < 0"; return ORBX_BAD_ARGUMENT; }
        if (M.n > 0 && (!M.in_view || !M.proj || !M.level || !M.view_cos || !M.desc || !M.observations)) {
            *why = "null field of a map-point view";
            return ORBX_BAD_ARGUMENT;
        }
        for (int i = 0; i < M.n; ++i)
            if (M.in_view[i] && (M.level[i] < 0 || M.level[i] >= a.nlevels)) {
                *why = "level outside [0, nlevels) on a point in view";
                return ORBX_BAD_ARGUMENT;
            }
        plan.nq += (size_t)M.n;
    }
    return tp_layout(plan, why);
}

// cv::gemm 3x3 * 3x1 float special case (as orbx_search_by_projection_frame)
static inline float tp_gemm3(const float *a, const float *b, float c) {
    const float t = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    return (float)((double)t * 1.0 + (double)c * 1.0);
}

void orbx_track_frame_pack(int nproblems, const orbx_track_frame_problem *problems, const OrbxTrackPlan &plan, const float *scale,
                           float mb, uint8_t *dst) {
    DTrackProb *dp = (DTrackProb *)(dst + plan.o_prob);
    DTrackQ *dq = (DTrackQ *)(dst + plan.o_q);
    uint8_t *dd = dst + plan.o_desc;
    size_t base = 0;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_track_frame_problem &P = problems[k];
        const orbx_last_frame_view &L = P.last;
        DTrackProb &D = dp[k];
        D.frame = P.frame; D.q_begin = (int32_t)base; D.nq = L.n;
        // twc = -Rcw.t() * tcw, tlc = Rlw * twc + tlw (src/ORBmatcher.cc:1722-1729): the direction of motion
        float Rlw[9], tlw[3], twc[3], tlc[3];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) { D.Rcw[3 * r + c] = P.Tcw[4 * r + c]; Rlw[3 * r + c] = L.Tcw[4 * r + c]; }
            D.tcw[r] = P.Tcw[4 * r + 3]; tlw[r] = L.Tcw[4 * r + 3];
        }
        for (int r = 0; r < 3; ++r) {
            const float t = D.Rcw[0 + r] * D.tcw[0] + D.Rcw[3 + r] * D.tcw[1] + D.Rcw[6 + r] * D.tcw[2];
            twc[r] = (float)((double)t * -1.0);
        }
        for (int r = 0; r < 3; ++r) tlc[r] = tp_gemm3(&Rlw[3 * r], twc, tlw[r]);
        const bool bForward = tlc[2] > mb && !P.mono, bBackward = -tlc[2] > mb && !P.mono;
        D.dir = bForward ? 1 : bBackward ? 2 : 0;
        for (int i = 0; i < L.n; ++i) {
            DTrackQ &Q = dq[base + i];
            const int oct = L.keys_un[i].octave;
            Q.x = L.world_pos[3 * (size_t)i]; Q.y = L.world_pos[3 * (size_t)i + 1]; Q.ur = L.world_pos[3 * (size_t)i + 2];
            Q.r = L.has_map_point[i] ? P.th * scale[oct] : -1.0f;   // the plan checked the octave of every such point
            Q.min_level = oct; Q.max_level = -1;
            Q.obs = L.observations[i];
            Q.angle = L.keys_un[i].angle;
            Q.prob = k; Q.pad = 0;
        }
        if (L.n > 0) memcpy(dd + base * 32, L.mp_desc, (size_t)L.n * 32);
        base += (size_t)L.n;
    }
}

void orbx_track_points_pack(int nproblems, const orbx_track_points_problem *problems, const OrbxTrackPlan &plan, const float *scale,
                            int cap, uint8_t *dst) {
    DTrackProb *dp = (DTrackProb *)(dst + plan.o_prob);
    DTrackQ *dq = (DTrackQ *)(dst + plan.o_q);
    uint8_t *dd = dst + plan.o_desc;
    uint32_t *ds = (uint32_t *)(dst + plan.o_seed);
    size_t base = 0;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_track_points_problem &P = problems[k];
        const orbx_mappoint_view &M = P.points;
        DTrackProb &D = dp[k];
        memset(&D, 0, sizeof(D));
        D.frame = P.frame; D.q_begin = (int32_t)base; D.nq = M.n;
        const bool bFactor = P.th != 1.0;
        for (int i = 0; i < M.n; ++i) {
            DTrackQ &Q = dq[base + i];
            Q.x = M.proj[3 * (size_t)i]; Q.y = M.proj[3 * (size_t)i + 1]; Q.ur = M.proj[3 * (size_t)i + 2];
            Q.r = -1.0f; Q.min_level = Q.max_level = -1;
            if (M.in_view[i]) {
                const int lvl = M.level[i];
                float r = M.view_cos[i] > 0.998 ? 2.5f : 4.0f;   // RadiusByViewingCos (src/ORBmatcher.cc:187-194)
                if (bFactor) r *= P.th;
                Q.r = r * scale[lvl];
                Q.min_level = lvl - 1; Q.max_level = lvl;
            }
            Q.obs = M.observations[i];
            Q.angle = 0.f;
            Q.prob = k; Q.pad = 0;
        }
        if (M.n > 0) memcpy(dd + base * 32, M.desc, (size_t)M.n * 32);
        uint32_t *seed = ds + (size_t)k * plan.seed_words;
        memset(seed, 0, (size_t)plan.seed_words * sizeof(uint32_t));
        if (P.frame_observations)
            for (int i = 0; i < cap; ++i)
                if (P.frame_observations[i] > 0) seed[i >> 5] |= 1u << (i & 31);
        base += (size_t)M.n;
    }
}

// ---------------------------------------------------------------- MapPoint::PredictScale as a table
// The reference's expression (src/MapPoint.cc:706-721 before the clamp, restated by tests/compat_runtime/map_model.cpp:
// ClampedScale), evaluated with this process's libm.  Only called with positive finite ratios: the quotient is finite and far
// inside int (|logf| <= 104, logf(scale_factor) >= 2^-24).
static inline int tp_raw_scale(float ratio, float log_scale_factor) {
    return (int)ceilf(logf(ratio) / log_scale_factor);
}

void orbx_predict_scale_build(float scale_factor, int nlevels, float *thr) {
    const float lsf = logf(scale_factor);
    const float inf = std::numeric_limits<float>::infinity();
    thr[0] = 0.f;
    for (int k = 1; k < ORBX_PS_LEVELS; ++k) {
        thr[k] = inf;
        if (k >= nlevels) continue;
        // bisection over the bit patterns of the positive finite floats (ascending with the value): lo gives < k, hi gives >= k
        uint32_t lo = 0x00000001u, hi = 0x7f7fffffu;
        float f;
        memcpy(&f, &hi, 4);
        if (tp_raw_scale(f, lsf) < k) continue;          // no finite ratio reaches level k
        memcpy(&f, &lo, 4);
        if (tp_raw_scale(f, lsf) >= k) { thr[k] = f; continue; }
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            memcpy(&f, &mid, 4);
            if (tp_raw_scale(f, lsf) >= k) hi = mid; else lo = mid;
        }
        memcpy(&thr[k], &hi, 4);
    }
}

// ---------------------------------------------------------------- orbx_search_local_points_batch_device
orbx_status orbx_track_local_plan(int nproblems, const orbx_track_local_problem *problems, const orbx_local_map_view *map,
                                  const OrbxTrackBatchArgs &a, OrbxLocalPlan &plan, const char **why) {
    plan = OrbxLocalPlan();
    const orbx_status st = tp_common(nproblems, problems, a, why);
    if (st != ORBX_OK) return st;
    const int npool = map ? map->n : 0;
    if (npool < 0) { *why = "map.n < 0"; return ORBX_BAD_ARGUMENT; }
    if (npool > 0 && (!map->world_pos || !map->normal || !map->min_distance || !map->max_distance || !map->desc ||
                      !map->observations)) {
        *why = "null field of a local-map view";
        return ORBX_BAD_ARGUMENT;
    }
    plan.nproblems = nproblems;
    plan.npool = npool;
    plan.seed_words = (a.cap + 31) / 32;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_track_local_problem &P = problems[k];
        if (P.frame < 0 || P.frame >= a.nframes) { *why = "frame outside [0, nframes)"; return ORBX_BAD_ARGUMENT; }
        if (P.npoints < 0) { *why = "npoints < 0"; return ORBX_BAD_ARGUMENT; }
        if (P.npoints > 0 && !map) { *why = "null local map with a non-empty problem"; return ORBX_BAD_ARGUMENT; }
        if (P.point_index) {
            for (int i = 0; i < P.npoints; ++i)
                if (P.point_index[i] < 0 || P.point_index[i] >= npool) { *why = "point_index outside the pool"; return ORBX_BAD_ARGUMENT; }
        } else if (P.npoints != 0 && P.npoints != npool) {
            *why = "point_index is NULL and npoints is not the pool's n";
            return ORBX_BAD_ARGUMENT;
        }
        if (P.npoints > plan.max_points) plan.max_points = P.npoints;
        plan.nq += (size_t)P.npoints;
    }
    if (plan.nq > (size_t)0x7fffffff / 64 || (size_t)npool > (size_t)0x7fffffff / 64) {
        *why = "too many points for 32-bit offsets";
        return ORBX_UNSUPPORTED;
    }
    OrbxLocalPlan &p = plan;
    p.o_prob = 0;
    p.o_local = tp_pad256((size_t)p.nproblems * sizeof(DTrackProb));
    p.o_pool = p.o_local + tp_pad256((size_t)p.nproblems * sizeof(DTrackLocal));
    p.o_pdesc = p.o_pool + tp_pad256((size_t)npool * sizeof(DTrackPoolPt));
    p.o_index = p.o_pdesc + tp_pad256((size_t)npool * 32);
    p.o_skip = p.o_index + tp_pad256(p.nq * sizeof(int32_t));
    p.o_seed = p.o_skip + tp_pad256(p.nq);
    p.in_bytes = p.o_seed + tp_pad256((size_t)p.nproblems * p.seed_words * sizeof(uint32_t));
    p.o_q = p.in_bytes;
    p.o_desc = p.o_q + tp_pad256(p.nq * sizeof(DTrackQ));
    p.o_cand = p.o_desc + tp_pad256(p.nq * 32);
    p.o_ev = p.o_cand + tp_pad256(p.nq * 16);
    p.dev_bytes = p.o_ev + tp_pad256(p.nq * sizeof(int32_t));
    return ORBX_OK;
}

void orbx_track_local_pack(int nproblems, const orbx_track_local_problem *problems, const orbx_local_map_view *map,
                           const OrbxLocalPlan &plan, int cap, uint8_t *dst) {
    DTrackProb *dp = (DTrackProb *)(dst + plan.o_prob);
    DTrackLocal *dl = (DTrackLocal *)(dst + plan.o_local);
    DTrackPoolPt *pool = (DTrackPoolPt *)(dst + plan.o_pool);
    int32_t *di = (int32_t *)(dst + plan.o_index);
    uint8_t *dk = dst + plan.o_skip;
    uint32_t *ds = (uint32_t *)(dst + plan.o_seed);
    for (int i = 0; i < plan.npool; ++i) {
        DTrackPoolPt &T = pool[i];
        for (int c = 0; c < 3; ++c) { T.P[c] = map->world_pos[3 * (size_t)i + c]; T.Pn[c] = map->normal[3 * (size_t)i + c]; }
        T.dmin = map->min_distance[i]; T.dmax = map->max_distance[i];
        T.obs = map->observations[i];
    }
    if (plan.npool > 0) memcpy(dst + plan.o_pdesc, map->desc, (size_t)plan.npool * 32);
    size_t base = 0;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_track_local_problem &P = problems[k];
        DTrackProb &D = dp[k];
        memset(&D, 0, sizeof(D));
        D.frame = P.frame; D.q_begin = (int32_t)base; D.nq = P.npoints;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) D.Rcw[3 * r + c] = P.Tcw[4 * r + c];
            D.tcw[r] = P.Tcw[4 * r + 3];
        }
        DTrackLocal &E = dl[k];
        memset(&E, 0, sizeof(E));
        for (int c = 0; c < 3; ++c) E.Ow[c] = P.Ow[c];
        E.th = P.th; E.cos_limit = P.viewing_cos_limit;
        for (int i = 0; i < P.npoints; ++i) {
            di[base + i] = P.point_index ? P.point_index[i] : i;
            dk[base + i] = P.skip && P.skip[i] ? 1 : 0;
        }
        uint32_t *seed = ds + (size_t)k * plan.seed_words;
        memset(seed, 0, (size_t)plan.seed_words * sizeof(uint32_t));
        if (P.frame_observations)
            for (int i = 0; i < cap; ++i)
                if (P.frame_observations[i] > 0) seed[i >> 5] |= 1u << (i & 31);
        base += (size_t)P.npoints;
    }
}
