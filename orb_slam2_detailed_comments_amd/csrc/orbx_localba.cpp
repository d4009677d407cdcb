// orbx_localba.cpp -- host side of the batched Optimizer::LocalBundleAdjustment (orbx_localba.h): validation of a call, the packing
// of all problems into one staging block with the two derived index lists (edges by free keyframe; the Schur blocks' pair
// entries), the library's host path -- the header's phases run by a plain loop over the same packed block, the problems one
// after the other -- and the scatter of the result block.  HIP-free: tools/san_localba.cpp builds it alone under the sanitizers.
// The entry points (orbx_map_batches.cpp) own the staging block and the launch.
#include <cstring>
#include "orbx_localba.h"

orbx_status orbx_localba_plan(int nproblems, const orbx_localba_problem *problems, const orbx_localba_result *results,
                              const orbx_localba_debug *dbg, bool debug, OrbxLbaPlan &plan, std::vector<DLbaProb> &probs, const char **why) {
    plan = OrbxLbaPlan();
    probs.clear();
    if (nproblems < 0) { *why = "nproblems < 0"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !problems) { *why = "null problem array"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !results) { *why = "null result array"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && debug && !dbg) { *why = "null state array"; return ORBX_BAD_ARGUMENT; }
    probs.resize((size_t)nproblems);
    std::vector<int32_t> seen;
    size_t in = orbx_pad256((size_t)nproblems * sizeof(DLbaProb)), work = 0;
    size_t out = orbx_pad256((size_t)nproblems * sizeof(orbx_localba_result));   // the output block starts with the results
    for (int k = 0; k < nproblems; ++k) {
        const orbx_localba_problem &P = problems[k];
        if (P.nlocal < 0 || P.nfixed < 0 || P.npoints < 0) { *why = "a negative count"; return ORBX_BAD_ARGUMENT; }
        if (P.nlocal > ORBX_LBA_MAX_LOCAL) { *why = "nlocal > 128 (the reduced system's workspace holds 768 x 768)"; return ORBX_UNSUPPORTED; }
        const int nkf = P.nlocal + P.nfixed;
        if (nkf < P.nlocal) { *why = "too many keyframes"; return ORBX_UNSUPPORTED; }
        if (nkf > 0 && !P.Tcw) { *why = "null Tcw"; return ORBX_BAD_ARGUMENT; }
        if (P.nlocal > 0 && !P.local_fixed) { *why = "null local_fixed"; return ORBX_BAD_ARGUMENT; }
        if (P.nlocal > 0 && !debug && !P.Tcw_out) { *why = "null Tcw_out"; return ORBX_BAD_ARGUMENT; }
        if (P.npoints > 0 && (!P.world || (!debug && !P.world_out))) { *why = "null world or world_out"; return ORBX_BAD_ARGUMENT; }
        if (!P.obs_begin) { *why = "null obs_begin"; return ORBX_BAD_ARGUMENT; }
        if (P.obs_begin[0] != 0) { *why = "obs_begin[0] != 0"; return ORBX_BAD_ARGUMENT; }
        for (int p = 0; p < P.npoints; ++p)
            if (P.obs_begin[p + 1] < P.obs_begin[p]) { *why = "obs_begin decreases"; return ORBX_BAD_ARGUMENT; }
        const int nobs = P.obs_begin[P.npoints];
        if (nobs > ORBX_LBA_MAX_OBS) { *why = "more than 4000000 observations in a problem"; return ORBX_UNSUPPORTED; }
        if (nobs > 0 && (!P.obs_kf || !P.obs || !P.inv_sigma2 || !P.erase)) { *why = "null obs_kf, obs, inv_sigma2 or erase"; return ORBX_BAD_ARGUMENT; }
        if (debug) {
            const orbx_localba_debug &D = dbg[k];
            if (nkf > 0 && (!D.Tcw_est || !D.Tcw_last)) { *why = "null Tcw_est or Tcw_last"; return ORBX_BAD_ARGUMENT; }
            if (P.npoints > 0 && (!D.world_est || !D.world_last)) { *why = "null world_est or world_last"; return ORBX_BAD_ARGUMENT; }
        }
        for (int e = 0; e < nobs; ++e)
            if (P.obs_kf[e] < 0 || P.obs_kf[e] >= nkf) { *why = "obs_kf outside the keyframe list"; return ORBX_BAD_ARGUMENT; }
        std::vector<int32_t> fcol((size_t)nkf, -1);
        int nfree = 0;
        for (int i = 0; i < P.nlocal; ++i) if (!P.local_fixed[i]) fcol[i] = nfree++;
        seen.assign((size_t)nkf, -1);
        size_t nkfe = 0, nent = 0;
        for (int p = 0; p < P.npoints; ++p) {
            size_t m = 0;
            for (int e = P.obs_begin[p]; e < P.obs_begin[p + 1]; ++e) {
                const int kf = P.obs_kf[e];
                if (seen[kf] == p) { *why = "a point lists one keyframe twice"; return ORBX_BAD_ARGUMENT; }
                seen[kf] = p;
                if (fcol[kf] >= 0) ++m;
            }
            nkfe += m;
            nent += m * (m + 1) / 2;
        }
        if (nent > (size_t)ORBX_LBA_MAX_ENT) { *why = "too many Schur pair entries in a problem"; return ORBX_UNSUPPORTED; }
        DLbaProb &D = probs[k];
        memset(&D, 0, sizeof(D));
        D.nlocal = P.nlocal; D.nfixed = P.nfixed; D.npoints = P.npoints; D.nobs = nobs; D.nfree = nfree;
        D.nkfe = (int32_t)nkfe; D.nent = (int32_t)nent; D.second_round = P.second_round ? 1 : 0;
        memcpy(D.cam, P.camera, sizeof(D.cam));
        D.bf = P.bf; D.debug = debug ? 1 : 0;
        OrbxLbaCtx c;
        const OrbxLbaSizes s = orbx_localba_bind(D, nullptr, nullptr, nullptr, c);
        D.o_in = (int64_t)in; D.o_work = (int64_t)work; D.o_out = (int64_t)out;
        in += s.in_bytes; work += s.work_bytes; out += s.out_bytes;
    }
    plan.nproblems = nproblems;
    plan.in_bytes = in; plan.work_bytes = work; plan.out_bytes = out;
    return ORBX_OK;
}

void orbx_localba_pack(const orbx_localba_problem *problems, const orbx_localba_debug *dbg, const OrbxLbaPlan &plan,
                       const std::vector<DLbaProb> &probs, uint8_t *dst) {
    if (plan.nproblems > 0) memcpy(dst + plan.o_prob, probs.data(), (size_t)plan.nproblems * sizeof(DLbaProb));
    std::vector<int32_t> cnt, pos, fl;
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_localba_problem &P = problems[k];
        const DLbaProb &D = probs[k];
        OrbxLbaCtx c;
        orbx_localba_bind(D, dst + D.o_in, nullptr, nullptr, c);
        const int nkf = c.nkf, np = c.npoints, no = c.nobs, nf = c.nfree;
        if (nkf) memcpy((void *)c.Tcw, P.Tcw, 16 * sizeof(float) * (size_t)nkf);
        if (np) memcpy((void *)c.world, P.world, 3 * sizeof(float) * (size_t)np);
        if (no) {
            memcpy((void *)c.obs, P.obs, 3 * sizeof(float) * (size_t)no);
            memcpy((void *)c.w, P.inv_sigma2, sizeof(float) * (size_t)no);
            memcpy((void *)c.obs_kf, P.obs_kf, sizeof(int32_t) * (size_t)no);
        }
        memcpy((void *)c.obs_begin, P.obs_begin, sizeof(int32_t) * ((size_t)np + 1));
        int32_t *edge_pt = (int32_t *)c.edge_pt, *fcol = (int32_t *)c.fcol, *free_kf = (int32_t *)c.free_kf;
        int32_t *kf_begin = (int32_t *)c.kf_begin, *kf_edge = (int32_t *)c.kf_edge;
        int32_t *blk_begin = (int32_t *)c.blk_begin, *blk_ij = (int32_t *)c.blk_ij, *blk_ent = (int32_t *)c.blk_ent;
        for (int i = 0, f = 0; i < nkf; ++i) {
            fcol[i] = i < P.nlocal && !P.local_fixed[i] ? f : -1;
            if (fcol[i] >= 0) free_kf[f++] = i;
        }
        for (int p = 0; p < np; ++p)
            for (int e = P.obs_begin[p]; e < P.obs_begin[p + 1]; ++e) edge_pt[e] = p;
        // edges by free keyframe, ascending edge index
        cnt.assign((size_t)nf + 1, 0);
        for (int e = 0; e < no; ++e) if (fcol[P.obs_kf[e]] >= 0) ++cnt[(size_t)fcol[P.obs_kf[e]] + 1];
        for (int f = 0; f < nf; ++f) cnt[(size_t)f + 1] += cnt[f];
        for (int f = 0; f <= nf; ++f) kf_begin[f] = cnt[f];
        pos.assign(cnt.begin(), cnt.end());
        for (int e = 0; e < no; ++e) { const int f = fcol[P.obs_kf[e]]; if (f >= 0) kf_edge[pos[f]++] = e; }
        // Schur blocks (i1 <= i2), i1-major; per block the (edge on i1, edge on i2) pairs of every point that has both, points
        // ascending
        const int nblk = c.nblk;
        auto blk = [nf](int i1, int i2) { return i1 * nf - (i1 * (i1 - 1)) / 2 + (i2 - i1); };
        for (int i1 = 0; i1 < nf; ++i1)
            for (int i2 = i1; i2 < nf; ++i2) { blk_ij[2 * blk(i1, i2)] = i1; blk_ij[2 * blk(i1, i2) + 1] = i2; }
        cnt.assign((size_t)nblk + 1, 0);
        for (int pass = 0; pass < 2; ++pass) {
            for (int p = 0; p < np; ++p) {
                fl.clear();
                for (int e = P.obs_begin[p]; e < P.obs_begin[p + 1]; ++e) if (fcol[P.obs_kf[e]] >= 0) fl.push_back(e);
                for (size_t a = 0; a < fl.size(); ++a)
                    for (size_t b = 0; b < fl.size(); ++b) {
                        const int i1 = fcol[P.obs_kf[fl[a]]], i2 = fcol[P.obs_kf[fl[b]]];
                        if (i1 > i2 || (i1 == i2 && a != b)) continue;
                        const int bi = blk(i1, i2);
                        if (pass == 0) { ++cnt[(size_t)bi + 1]; continue; }
                        const int at = pos[bi]++;
                        blk_ent[2 * at] = fl[a]; blk_ent[2 * at + 1] = fl[b];
                    }
            }
            if (pass == 0) {
                for (int b = 0; b < nblk; ++b) cnt[(size_t)b + 1] += cnt[b];
                for (int b = 0; b <= nblk; ++b) blk_begin[b] = cnt[b];
                pos.assign(cnt.begin(), cnt.end());
            }
        }
        if (D.debug) {
            float *g = (float *)c.dbg;
            const size_t a = 16 * (size_t)nkf, b = 3 * (size_t)np;
            if (a) { memcpy(g, dbg[k].Tcw_est, a * sizeof(float)); memcpy(g + a + b, dbg[k].Tcw_last, a * sizeof(float)); }
            if (b) { memcpy(g + a, dbg[k].world_est, b * sizeof(float)); memcpy(g + 2 * a + b, dbg[k].world_last, b * sizeof(float)); }
        }
    }
}

namespace {
struct LbaExHost {
    template <class F> void each(int n, F f) { for (int i = 0; i < n; ++i) f(i); }
    void sync() {}
    bool lead() const { return true; }
};
}  // namespace

void orbx_localba_host_run(const OrbxLbaPlan &plan, const uint8_t *in, uint8_t *work, uint8_t *out) {
    orbx_localba_result *res = (orbx_localba_result *)out;
    const DLbaProb *dp = (const DLbaProb *)(in + plan.o_prob);
    for (int k = 0; k < plan.nproblems; ++k) {
        OrbxLbaCtx c;
        orbx_localba_bind(dp[k], in + dp[k].o_in, work + dp[k].o_work, out + dp[k].o_out, c);
        LbaExHost ex;
        orbx_localba_run(ex, c, &res[k]);
    }
}

void orbx_localba_unpack(const orbx_localba_problem *problems, const std::vector<DLbaProb> &probs, const uint8_t *out, bool debug,
                         orbx_localba_result *results) {
    const orbx_localba_result *res = (const orbx_localba_result *)out;
    for (size_t k = 0; k < probs.size(); ++k) {
        const orbx_localba_problem &P = problems[k];
        OrbxLbaCtx c;
        orbx_localba_bind(probs[k], nullptr, nullptr, (uint8_t *)out + probs[k].o_out, c);
        results[k] = res[k];
        if (c.nobs) memcpy(P.erase, c.erase, (size_t)c.nobs);
        if (debug) continue;
        if (c.nlocal) memcpy(P.Tcw_out, c.Tcw_out, 16 * sizeof(float) * (size_t)c.nlocal);
        if (c.npoints) memcpy(P.world_out, c.world_out, 3 * sizeof(float) * (size_t)c.npoints);
    }
}
