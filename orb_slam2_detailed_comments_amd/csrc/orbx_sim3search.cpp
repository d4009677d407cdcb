// orbx_sim3search.cpp -- host side of the batched ORBmatcher::SearchBySim3 (orbx_sim3search.h): validation of a call, the
// packing of the keyframe pool and the problems into one staging block (each keyframe once, the per-problem similarity worked
// out while packing), the library's host path -- the header's scalar code over the same packed block with the Frame grid and
// the reference's bucket walk -- and the scatter of the result block.  HIP-free: tests/san_sim3search.cpp builds it alone
// under the sanitizers.  The entry point (orbx_map_batches.cpp) owns the staging block and the launches.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "orbx_sim3search.h"

static const char *keyframe_fault(const orbx_sim3_search_keyframe &K, int nlevels, bool *unsupported) {
    if (K.n < 0) return "a negative feature count";
    if (K.n > 65535) { *unsupported = true; return "more than 65535 features in a keyframe (16-bit bucket entries and visiting positions)"; }
    if (K.n == 0) return nullptr;
    if (!K.keys_un || !K.desc || !K.has_point || !K.world_pos || !K.min_distance || !K.max_distance || !K.point_desc)
        return "a null field of a non-empty keyframe";
    for (int i = 0; i < K.n; ++i)
        if (K.keys_un[i].octave < 0 || K.keys_un[i].octave >= nlevels) return "an octave outside [0, nlevels)";
    return nullptr;
}

orbx_status orbx_sim3s_plan(int nkeyframes, const orbx_sim3_search_keyframe *keyframes, int nproblems,
                            const orbx_sim3_search_problem *problems, const float *camera4, const float *bounds4, int nlevels,
                            int32_t *const *matches12, const int *nfound, OrbxSim3sPlan &plan, const char **why) {
    plan = OrbxSim3sPlan();
    if (nkeyframes < 0) { *why = "nkeyframes < 0"; return ORBX_BAD_ARGUMENT; }
    if (nproblems < 0) { *why = "nproblems < 0"; return ORBX_BAD_ARGUMENT; }
    if (nkeyframes > 0 && !keyframes) { *why = "null keyframe array"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && (!problems || !matches12 || !nfound || !camera4 || !bounds4)) {
        *why = "null problems, matches12, nfound, camera4 or bounds4"; return ORBX_BAD_ARGUMENT;
    }
    if (nlevels < 1 || nlevels > ORBX_PS_LEVELS) { *why = "level count of the handle"; return ORBX_BAD_ARGUMENT; }
    int fstride = 0;
    for (int f = 0; f < nkeyframes; ++f) {
        bool unsupported = false;
        const char *fault = keyframe_fault(keyframes[f], nlevels, &unsupported);
        if (fault) { *why = fault; return unsupported ? ORBX_UNSUPPORTED : ORBX_BAD_ARGUMENT; }
        if (keyframes[f].n > fstride) fstride = keyframes[f].n;
    }
    size_t nq = 0, nm = 0;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_sim3_search_problem &P = problems[k];
        if (P.kf1 < 0 || P.kf1 >= nkeyframes || P.kf2 < 0 || P.kf2 >= nkeyframes) { *why = "kf1 or kf2 outside the pool"; return ORBX_BAD_ARGUMENT; }
        const int n1 = keyframes[P.kf1].n, n2 = keyframes[P.kf2].n;
        if (n1 > 0 && !matches12[k]) { *why = "a null matches12 row"; return ORBX_BAD_ARGUMENT; }
        nq += (size_t)n1 + (size_t)n2;
        nm += (size_t)n1;
    }
    if (nproblems > 0 && (!(bounds4[1] > bounds4[0]) || !(bounds4[3] > bounds4[2]))) { *why = "bad image bounds"; return ORBX_BAD_ARGUMENT; }
    if (nq > (size_t)0x3fffffff) { *why = "too many features for 32-bit offsets"; return ORBX_UNSUPPORTED; }
    plan.nkf = nkeyframes; plan.nproblems = nproblems; plan.fstride = fstride; plan.max_n = fstride;
    plan.nq = nq; plan.nm = nm;
    const size_t nrec = (size_t)nkeyframes * (size_t)fstride;
    plan.o_ctr = 0;
    plan.o_cnt = 256;
    plan.o_prob = plan.o_cnt + orbx_pad256((size_t)nkeyframes * sizeof(int32_t));
    plan.o_keys = plan.o_prob + orbx_pad256((size_t)nproblems * sizeof(DSim3sProb));
    plan.o_desc = plan.o_keys + orbx_pad256(nrec * sizeof(orbx_keypoint));
    plan.o_pt = plan.o_desc + orbx_pad256(nrec * 32);
    plan.o_pdesc = plan.o_pt + orbx_pad256(nrec * sizeof(DSim3sPt));
    plan.o_flag = plan.o_pdesc + orbx_pad256(nrec * 32);
    plan.in_bytes = plan.o_flag + orbx_pad256(nq);
    plan.o_cb = 0;
    plan.o_it = plan.o_cb + orbx_pad256((size_t)nkeyframes * (ORBX_SIM3S_GRID_CELLS + 1) * sizeof(int32_t));
    plan.o_q = plan.o_it + orbx_pad256(nrec * sizeof(uint16_t));
    plan.o_live = plan.o_q + orbx_pad256(nq * sizeof(DTrackQ));
    plan.o_out = plan.o_live + orbx_pad256(nq * sizeof(int32_t));
    plan.o_nf = 0;
    plan.o_m = orbx_pad256((size_t)nproblems * sizeof(int32_t));
    plan.out_small = plan.o_m + orbx_pad256(nm * sizeof(int32_t));
    plan.o_best = plan.out_small;
    plan.o_level = plan.o_best + orbx_pad256(nq * sizeof(int32_t));
    plan.o_uv = plan.o_level + orbx_pad256(nq * sizeof(int32_t));
    plan.o_status = plan.o_uv + orbx_pad256(nq * 2 * sizeof(float));
    plan.out_bytes = plan.o_status + orbx_pad256(nq);
    plan.dev_bytes = plan.o_out + plan.out_bytes;
    return ORBX_OK;
}

void orbx_sim3s_camera(const float *camera4, const float *bounds4, int fma_mode, int nlevels, const float *thr, const float *scale,
                       OrbxSim3sCam &cam, OrbxSim3sGrid &grid) {
    cam.fx = camera4[0]; cam.fy = camera4[1]; cam.cx = camera4[2]; cam.cy = camera4[3];
    cam.minx = bounds4[0]; cam.maxx = bounds4[1]; cam.miny = bounds4[2]; cam.maxy = bounds4[3];
    cam.fma_mode = fma_mode; cam.nlevels = nlevels;
    for (int l = 0; l < ORBX_PS_LEVELS; ++l) { cam.thr[l] = thr[l]; cam.scale[l] = l < nlevels ? scale[l] : 0.0f; }
    grid.minx = bounds4[0]; grid.miny = bounds4[2];
    grid.winv = 64.0f / (bounds4[1] - bounds4[0]);     // mfGridElementWidthInv (src/Frame.cc:96-99)
    grid.hinv = 48.0f / (bounds4[3] - bounds4[2]);
}

void orbx_sim3s_pack(const orbx_sim3_search_keyframe *keyframes, const orbx_sim3_search_problem *problems, const OrbxSim3sPlan &plan,
                     uint8_t *dst) {
    memset(dst + plan.o_ctr, 0, 256);
    int32_t *cnt = (int32_t *)(dst + plan.o_cnt);
    const size_t fs = (size_t)plan.fstride;
    for (int f = 0; f < plan.nkf; ++f) {
        const orbx_sim3_search_keyframe &K = keyframes[f];
        cnt[f] = K.n;
        if (K.n == 0) continue;
        memcpy(dst + plan.o_keys + f * fs * sizeof(orbx_keypoint), K.keys_un, (size_t)K.n * sizeof(orbx_keypoint));
        memcpy(dst + plan.o_desc + f * fs * 32, K.desc, (size_t)K.n * 32);
        DSim3sPt *pt = (DSim3sPt *)(dst + plan.o_pt) + f * fs;
        uint8_t *pd = dst + plan.o_pdesc + f * fs * 32;
        for (int i = 0; i < K.n; ++i) {
            DSim3sPt &T = pt[i];
            memset(&T, 0, sizeof(T));
            if (!K.has_point[i]) { memset(pd + (size_t)i * 32, 0, 32); continue; }
            T.has = 1;
            T.P[0] = K.world_pos[3 * (size_t)i]; T.P[1] = K.world_pos[3 * (size_t)i + 1]; T.P[2] = K.world_pos[3 * (size_t)i + 2];
            T.dmin = K.min_distance[i]; T.dmax = K.max_distance[i];
            memcpy(pd + (size_t)i * 32, K.point_desc + (size_t)i * 32, 32);
        }
    }
    DSim3sProb *dp = (DSim3sProb *)(dst + plan.o_prob);
    uint8_t *flag = dst + plan.o_flag;
    size_t q = 0, m = 0;
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_sim3_search_problem &P = problems[k];
        DSim3sProb &D = dp[k];
        memset(&D, 0, sizeof(D));
        D.kf[0] = P.kf1; D.kf[1] = P.kf2;
        D.n[0] = keyframes[P.kf1].n; D.n[1] = keyframes[P.kf2].n;
        D.q_off = (int32_t)q; D.m_off = (int32_t)m; D.th = P.th;
        float sR12[9], sR21[9], t21[3];
        orbx_sim3s_similarity(P.s12, P.R12, P.t12, sR12, sR21, t21);
        for (int d = 0; d < 2; ++d) {
            const float *T = keyframes[D.kf[d]].Tcw;
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) D.dir[d].Rw[3 * r + c] = T[4 * r + c];
                D.dir[d].tw[r] = T[4 * r + 3];
            }
        }
        memcpy(D.dir[0].sR, sR21, sizeof(sR21)); memcpy(D.dir[0].t, t21, sizeof(t21));
        memcpy(D.dir[1].sR, sR12, sizeof(sR12)); memcpy(D.dir[1].t, P.t12, sizeof(t21));
        const uint8_t *src[2] = {P.matched1, P.matched2};
        for (int d = 0; d < 2; ++d) {
            uint8_t *f = flag + q + (d ? (size_t)D.n[0] : 0);
            if (D.n[d] > 0 && src[d]) memcpy(f, src[d], (size_t)D.n[d]);
            else if (D.n[d] > 0) memset(f, 0, (size_t)D.n[d]);
        }
        q += (size_t)D.n[0] + (size_t)D.n[1];
        m += (size_t)D.n[0];
    }
}

namespace {
// Frame::AssignFeaturesToGrid + PosInGrid (src/Frame.cc:432-460, 729-745) as k_grid_build leaves it: per bucket (ix * 48 + iy)
// the features in ascending index
struct HostGrid {
    std::vector<int32_t> cb;
    std::vector<uint16_t> items;
    static int cell_of(const OrbxSim3sGrid &g, const orbx_keypoint &kp) {
        const int px = (int)roundf((kp.x - g.minx) * g.winv), py = (int)roundf((kp.y - g.miny) * g.hinv);
        return (px < 0 || px >= ORBX_SIM3S_GRID_COLS || py < 0 || py >= ORBX_SIM3S_GRID_ROWS) ? -1 : px * ORBX_SIM3S_GRID_ROWS + py;
    }
    void build(const OrbxSim3sGrid &g, const orbx_keypoint *k, int n) {
        cb.assign(ORBX_SIM3S_GRID_CELLS + 1, 0);
        items.assign((size_t)(n > 0 ? n : 1), 0);
        for (int i = 0; i < n; ++i) { const int c = cell_of(g, k[i]); if (c >= 0) cb[(size_t)c + 1]++; }
        for (int c = 0; c < ORBX_SIM3S_GRID_CELLS; ++c) cb[(size_t)c + 1] += cb[(size_t)c];
        std::vector<int32_t> at(cb.begin(), cb.end() - 1);
        for (int i = 0; i < n; ++i) { const int c = cell_of(g, k[i]); if (c >= 0) items[(size_t)at[(size_t)c]++] = (uint16_t)i; }
    }
};
}  // namespace

void orbx_sim3s_host_run(const OrbxSim3sPlan &plan, const OrbxSim3sCam &cam, const OrbxSim3sGrid &g, const uint8_t *in, uint8_t *out) {
    const int32_t *cnt = (const int32_t *)(in + plan.o_cnt);
    const DSim3sProb *dp = (const DSim3sProb *)(in + plan.o_prob);
    const size_t fs = (size_t)plan.fstride;
    const orbx_keypoint *keys = (const orbx_keypoint *)(in + plan.o_keys);
    const uint8_t *desc = in + plan.o_desc, *pdesc = in + plan.o_pdesc, *flag = in + plan.o_flag;
    const DSim3sPt *pt = (const DSim3sPt *)(in + plan.o_pt);
    int32_t *nfound = (int32_t *)(out + plan.o_nf), *matches = (int32_t *)(out + plan.o_m), *best = (int32_t *)(out + plan.o_best),
            *level = (int32_t *)(out + plan.o_level);
    float *uv = (float *)(out + plan.o_uv);
    uint8_t *status = out + plan.o_status;
    std::vector<HostGrid> grids((size_t)plan.nkf);
    std::vector<uint8_t> built((size_t)plan.nkf, 0);
    for (int k = 0; k < plan.nproblems; ++k) {
        const DSim3sProb &D = dp[k];
        for (int d = 0; d < 2; ++d) {
            const int src = D.kf[d], tgt = D.kf[1 - d], nt = cnt[tgt];
            if (!built[(size_t)tgt]) { grids[(size_t)tgt].build(g, keys + tgt * fs, nt); built[(size_t)tgt] = 1; }
            const HostGrid &G = grids[(size_t)tgt];
            const orbx_keypoint *tk = keys + tgt * fs;
            const uint8_t *td = desc + tgt * fs * 32;
            const size_t q0 = (size_t)D.q_off + (d ? (size_t)D.n[0] : 0);
            for (int i = 0; i < D.n[d]; ++i) {
                const size_t gq = q0 + (size_t)i;
                const DSim3sPt &T = pt[src * fs + (size_t)i];
                best[gq] = -1; level[gq] = -1; uv[2 * gq] = 0.0f; uv[2 * gq + 1] = 0.0f;
                status[gq] = ORBX_SIM3S_NOT_SEARCHED;
                if (!T.has || flag[gq]) continue;
                const OrbxSim3sProj o = orbx_sim3s_project(D.dir[d], cam, D.th, T);
                status[gq] = (uint8_t)o.status; uv[2 * gq] = o.u; uv[2 * gq + 1] = o.v; level[gq] = o.level;
                if (o.status != ORBX_SIM3S_NO_CANDIDATE) continue;
                // KeyFrame::GetFeaturesInArea (src/KeyFrame.cc) and the loop of :1555-1573
                const float x = o.u, y = o.v, r = o.r;
                const int x0 = std::max(0, (int)floorf((x - g.minx - r) * g.winv));
                const int x1 = std::min(ORBX_SIM3S_GRID_COLS - 1, (int)ceilf((x - g.minx + r) * g.winv));
                const int y0 = std::max(0, (int)floorf((y - g.miny - r) * g.hinv));
                const int y1 = std::min(ORBX_SIM3S_GRID_ROWS - 1, (int)ceilf((y - g.miny + r) * g.hinv));
                uint32_t key = 0xffffffffu;
                int idx = -1;
                if (r >= 0.0f && x0 < ORBX_SIM3S_GRID_COLS && x1 >= 0 && y0 < ORBX_SIM3S_GRID_ROWS && y1 >= 0) {
                    const uint32_t *qd = (const uint32_t *)(pdesc + (src * fs + (size_t)i) * 32);
                    uint32_t pos = 0;
                    for (int ix = x0; ix <= x1; ++ix)
                        for (int iy = y0; iy <= y1; ++iy) {
                            const int c = ix * ORBX_SIM3S_GRID_ROWS + iy;
                            for (int j = G.cb[(size_t)c]; j < G.cb[(size_t)c + 1]; ++j, ++pos) {
                                const int i2 = G.items[(size_t)j];
                                const orbx_keypoint &kp = tk[i2];
                                if (!(fabsf(kp.x - x) < r && fabsf(kp.y - y) < r)) continue;
                                if (kp.octave < o.level - 1 || kp.octave > o.level) continue;
                                const uint32_t *t4 = (const uint32_t *)(td + (size_t)i2 * 32);
                                uint32_t dist = 0;
                                for (int w = 0; w < 8; ++w) dist += (uint32_t)__builtin_popcount(qd[w] ^ t4[w]);
                                const uint32_t kk = (dist << 16) | pos;
                                if (kk < key) { key = kk; idx = i2; }
                            }
                        }
                }
                status[gq] = (uint8_t)orbx_sim3s_outcome(key, idx, &best[gq]);
            }
        }
        int n = 0;
        for (int i1 = 0; i1 < D.n[0]; ++i1) {                       // the mutual test (:1667-1681)
            const int32_t idx2 = best[(size_t)D.q_off + (size_t)i1];
            const bool both = idx2 >= 0 && best[(size_t)D.q_off + (size_t)D.n[0] + (size_t)idx2] == i1;
            matches[(size_t)D.m_off + (size_t)i1] = both ? idx2 : -1;
            n += both ? 1 : 0;
        }
        nfound[k] = n;
    }
}

void orbx_sim3s_unpack(const OrbxSim3sPlan &plan, const uint8_t *in, const uint8_t *out,
                       int32_t *const *matches12, int *nfound, const orbx_sim3_search_debug *dbg) {
    const DSim3sProb *dp = (const DSim3sProb *)(in + plan.o_prob);
    const int32_t *nf = (const int32_t *)(out + plan.o_nf), *m = (const int32_t *)(out + plan.o_m);
    const int32_t *best = (const int32_t *)(out + plan.o_best), *level = (const int32_t *)(out + plan.o_level);
    const float *uv = (const float *)(out + plan.o_uv);
    const uint8_t *status = out + plan.o_status;
    for (int k = 0; k < plan.nproblems; ++k) {
        const DSim3sProb &D = dp[k];
        nfound[k] = nf[k];
        if (D.n[0] > 0) memcpy(matches12[k], m + D.m_off, (size_t)D.n[0] * sizeof(int32_t));
        if (!dbg) continue;
        for (int d = 0; d < 2; ++d) {
            const size_t q0 = (size_t)D.q_off + (d ? (size_t)D.n[0] : 0), n = (size_t)D.n[d];
            if (n == 0) continue;
            uint8_t *const *st = d ? dbg->status2 : dbg->status1;
            int32_t *const *be = d ? dbg->best2 : dbg->best1, *const *le = d ? dbg->level2 : dbg->level1;
            float *const *u = d ? dbg->uv2 : dbg->uv1;
            if (st && st[k]) memcpy(st[k], status + q0, n);
            if (be && be[k]) memcpy(be[k], best + q0, n * sizeof(int32_t));
            if (le && le[k]) memcpy(le[k], level + q0, n * sizeof(int32_t));
            if (u && u[k]) memcpy(u[k], uv + 2 * q0, n * 2 * sizeof(float));
        }
    }
}
