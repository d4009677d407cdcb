// orbx_sim3opt.cpp -- host side of the batched Optimizer::OptimizeSim3 (orbx_sim3opt.h): validation of a call, the packing of all
// problems into one staging block (per problem 12 planes of n floats), the library's host path -- the header's scalar code
// compiled by the host compiler over the same packed block, the problems one after the other and the edges of a problem in
// the order e12_i, e21_i for i ascending -- and the scatter of the result block.  HIP-free: tests/san_sim3opt.cpp builds it alone
// under the sanitizers.  The entry points (orbx_map_batches.cpp) own the staging block and the launch.
#include <cstring>
#include "orbx_sim3opt.h"

orbx_status orbx_sim3opt_plan(int nproblems, const orbx_sim3opt_problem *problems, const orbx_sim3opt_result *results,
                              const double *last, bool inlier_test, OrbxSim3OptPlan &plan, const char **why) {
    plan = OrbxSim3OptPlan();
    if (nproblems < 0) { *why = "nproblems < 0"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !problems) { *why = "null problem array"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !results) { *why = "null result array"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && inlier_test && !last) { *why = "null S_last array"; return ORBX_BAD_ARGUMENT; }
    size_t total = 0;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_sim3opt_problem &P = problems[k];
        if (P.n < 0) { *why = "n < 0"; return ORBX_BAD_ARGUMENT; }
        if (P.n == 0) continue;
        if (!P.x1c || !P.x2c) { *why = "null x1c or x2c"; return ORBX_BAD_ARGUMENT; }
        if (!P.obs1 || !P.obs2) { *why = "null obs1 or obs2"; return ORBX_BAD_ARGUMENT; }
        if (!P.inv_sigma2_1 || !P.inv_sigma2_2) { *why = "null inv_sigma2_1 or inv_sigma2_2"; return ORBX_BAD_ARGUMENT; }
        if (!P.keep) { *why = "null keep"; return ORBX_BAD_ARGUMENT; }
        total += (size_t)P.n;
    }
    if (total > (size_t)0x7fffffff / ORBX_SIM3OPT_PLANES) { *why = "too many correspondences for 32-bit offsets"; return ORBX_UNSUPPORTED; }
    plan.nproblems = nproblems;
    plan.total = total;
    plan.o_prob = 0;
    plan.o_pts = orbx_pad256((size_t)nproblems * sizeof(DSim3OptProb));
    plan.in_bytes = plan.o_pts + orbx_pad256(total * ORBX_SIM3OPT_PLANES * sizeof(float));
    plan.o_res = 0;
    plan.o_keep = orbx_pad256((size_t)nproblems * sizeof(orbx_sim3opt_result));
    plan.out_bytes = plan.o_keep + orbx_pad256(total);
    return ORBX_OK;
}

void orbx_sim3opt_pack(const orbx_sim3opt_problem *problems, const double *last, const OrbxSim3OptPlan &plan, uint8_t *dst) {
    DSim3OptProb *dp = (DSim3OptProb *)(dst + plan.o_prob);
    float *pts = (float *)(dst + plan.o_pts);
    size_t off = 0;
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_sim3opt_problem &P = problems[k];
        DSim3OptProb &D = dp[k];
        D.n = P.n; D.fix_scale = P.fix_scale ? 1 : 0; D.off = (int64_t)off;
        memcpy(D.cam1, P.camera1, sizeof(D.cam1)); memcpy(D.cam2, P.camera2, sizeof(D.cam2));
        memcpy(D.R, P.R, sizeof(D.R)); memcpy(D.t, P.t, sizeof(D.t));
        D.s = P.s; D.th2 = P.th2;
        for (int j = 0; j < 8; ++j) D.last[j] = last ? last[8 * (size_t)k + j] : 0.0;
        const size_t n = (size_t)P.n;
        float *pl = pts + ORBX_SIM3OPT_PLANES * off;
        for (size_t i = 0; i < n; ++i) {
            for (int c = 0; c < 3; ++c) { pl[c * n + i] = P.x1c[3 * i + c]; pl[(3 + c) * n + i] = P.x2c[3 * i + c]; }
            for (int c = 0; c < 2; ++c) { pl[(6 + c) * n + i] = P.obs1[2 * i + c]; pl[(8 + c) * n + i] = P.obs2[2 * i + c]; }
            pl[10 * n + i] = P.inv_sigma2_1[i];
            pl[11 * n + i] = P.inv_sigma2_2[i];
        }
        off += n;
    }
}

namespace {
// The three passes of orbx_sim3opt_run over one problem's live correspondences, one after the other
struct Sim3OptEvHost {
    OrbxSim3OptView v;
    OrbxSim3OptCam K1, K2;
    double th2, delta;
    bool fix_scale;
    uint8_t *keep;
    void system(const OrbxSim3 &S, double *acc) const {
        double tab[ORBX_SIM3OPT_NSIM * ORBX_SIM3OPT_SIM], term[ORBX_SIM3OPT_TERMS];
        for (int k = 0; k < ORBX_SIM3OPT_NSIM; ++k) orbx_sim3opt_table_entry(S, k, fix_scale, tab + k * ORBX_SIM3OPT_SIM);
        for (int t = 0; t < ORBX_SIM3OPT_TERMS; ++t) acc[t] = 0.0;
        OrbxSim3OptEdge e12, e21;
        for (int i = 0; i < v.n; ++i) {
            if (!keep[i]) continue;
            orbx_sim3opt_load(v, i, e12, e21);
            orbx_sim3opt_terms(tab, 0, K1, e12, delta, term);
            for (int t = 0; t < ORBX_SIM3OPT_TERMS; ++t) acc[t] = orbx_lm_accumulate<7>(t, acc[t], term[t]);
            orbx_sim3opt_terms(tab, 8, K2, e21, delta, term);
            for (int t = 0; t < ORBX_SIM3OPT_TERMS; ++t) acc[t] = orbx_lm_accumulate<7>(t, acc[t], term[t]);
        }
    }
    double chi(const OrbxSim3 &S) const {
        double tab[ORBX_SIM3OPT_SIM], s = 0.0, err[2], rho1;
        orbx_sim3opt_table_entry(S, 0, fix_scale, tab);
        OrbxSim3OptEdge e12, e21;
        for (int i = 0; i < v.n; ++i) {
            if (!keep[i]) continue;
            orbx_sim3opt_load(v, i, e12, e21);
            s = s + orbx_lm_huber(orbx_sim3opt_error(tab, K1, e12, err), delta, &rho1);
            s = s + orbx_lm_huber(orbx_sim3opt_error(tab + 8, K2, e21, err), delta, &rho1);
        }
        return s;
    }
    OrbxSim3 oplus(const OrbxSim3 &S, double *x) const { return orbx_sim3opt_oplus(S, x, fix_scale); }
    int classify(const OrbxSim3 &Slast) {
        double tab[ORBX_SIM3OPT_SIM], err[2];
        orbx_sim3opt_table_entry(Slast, 0, fix_scale, tab);
        OrbxSim3OptEdge e12, e21;
        int nbad = 0;
        for (int i = 0; i < v.n; ++i) {
            if (!keep[i]) continue;
            orbx_sim3opt_load(v, i, e12, e21);
            const bool bad = orbx_sim3opt_error(tab, K1, e12, err) > th2 || orbx_sim3opt_error(tab + 8, K2, e21, err) > th2;
            if (bad) { keep[i] = 0; ++nbad; }
        }
        return nbad;
    }
};
}  // namespace

void orbx_sim3opt_host_run(const OrbxSim3OptPlan &plan, const uint8_t *in, bool inlier_test, uint8_t *out) {
    const DSim3OptProb *dp = (const DSim3OptProb *)(in + plan.o_prob);
    const float *pts = (const float *)(in + plan.o_pts);
    orbx_sim3opt_result *res = (orbx_sim3opt_result *)(out + plan.o_res);
    uint8_t *keep = out + plan.o_keep;
    for (int k = 0; k < plan.nproblems; ++k) {
        const DSim3OptProb &D = dp[k];
        Sim3OptEvHost ev;
        ev.v.pl = pts + ORBX_SIM3OPT_PLANES * (size_t)D.off;
        ev.v.n = D.n;
        ev.K1.fx = (double)D.cam1[0]; ev.K1.fy = (double)D.cam1[1]; ev.K1.cx = (double)D.cam1[2]; ev.K1.cy = (double)D.cam1[3];
        ev.K2.fx = (double)D.cam2[0]; ev.K2.fy = (double)D.cam2[1]; ev.K2.cx = (double)D.cam2[2]; ev.K2.cy = (double)D.cam2[3];
        ev.th2 = (double)D.th2;
        ev.delta = (double)(float)sqrt((double)D.th2);         // const float deltaHuber = sqrt(th2)
        ev.fix_scale = D.fix_scale != 0;
        ev.keep = keep + D.off;
        for (int i = 0; i < D.n; ++i) ev.keep[i] = 1;
        const OrbxSim3 init = orbx_sim3opt_from_input(D.R, D.t, D.s);
        if (inlier_test) {
            const int nbad = ev.classify(orbx_sim3opt_fetch(D.last));
            orbx_sim3opt_store_result(init, D.n - nbad, nbad, D.n, 0, &res[k]);
            continue;
        }
        orbx_sim3opt_run(ev, init, D.n, &res[k]);
    }
}

void orbx_sim3opt_unpack(const orbx_sim3opt_problem *problems, const OrbxSim3OptPlan &plan, const uint8_t *out, orbx_sim3opt_result *results) {
    const orbx_sim3opt_result *res = (const orbx_sim3opt_result *)(out + plan.o_res);
    const uint8_t *keep = out + plan.o_keep;
    size_t off = 0;
    for (int k = 0; k < plan.nproblems; ++k) {
        results[k] = res[k];
        if (problems[k].n > 0) memcpy(problems[k].keep, keep + off, (size_t)problems[k].n);
        off += (size_t)problems[k].n;
    }
}

extern "C" double orbx_sim3opt_exp(double sigma) { return orbx_sim3opt_expd(sigma); }
