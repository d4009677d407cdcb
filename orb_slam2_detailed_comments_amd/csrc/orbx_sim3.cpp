// orbx_sim3.cpp -- host side of the batched Sim3Solver RANSAC (orbx_sim3.h): validation of a call, the packing of all problems
// into one staging block, the library's host path -- the header's scalar code compiled by the host compiler over that same
// block -- SetRansacParameters, and the iterate() cursor over the stored results.  HIP-free: tests/san_sim3.cpp builds it alone
// under the sanitizers.  The entry points (orbx_map_batches.cpp) own the staging block, the arena and the launches.
#include <cmath>
#include <cstring>
#include <algorithm>
#include "orbx_sim3.h"

static inline bool sim3_launches(const orbx_sim3_problem &P) { return P.n >= P.min_inliers; }
static inline OrbxRansacWalk sim3_walk(int32_t *hyp_prob = nullptr, int32_t *groups = nullptr) {
    return OrbxRansacWalk(0x3fffffff, SIZE_MAX, hyp_prob, groups);   // no limit on the set ints: no record stores an offset into them
}
static inline OrbxRansacWalk::At sim3_add(OrbxRansacWalk &w, const orbx_sim3_problem &P) {
    return w.add(P.n, (size_t)P.iterations, (size_t)P.iterations * 3, ORBX_SIM3_PLANES, ORBX_SIM3_WAVES);
}

orbx_status orbx_sim3_plan(int nproblems, const orbx_sim3_problem *problems, OrbxSim3Plan &plan, const char **why) {
    plan = OrbxSim3Plan();
    if (nproblems < 0) { *why = "nproblems < 0"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !problems) { *why = "null problem array"; return ORBX_BAD_ARGUMENT; }
    OrbxRansacWalk w = sim3_walk();
    for (int k = 0; k < nproblems; ++k) {
        const orbx_sim3_problem &P = problems[k];
        if (P.n < 0) { *why = "n < 0"; return ORBX_BAD_ARGUMENT; }
        if (P.iterations < 1) { *why = "iterations < 1"; return ORBX_BAD_ARGUMENT; }
        if (P.n > 0 && (!P.x1c || !P.x2c || !P.max_err1 || !P.max_err2)) { *why = "null correspondence array with n > 0"; return ORBX_BAD_ARGUMENT; }
        if (!sim3_launches(P)) continue;
        if (!P.sets) { *why = "null sets"; return ORBX_BAD_ARGUMENT; }
        for (int i = 0; i < P.iterations; ++i)                 // a repeated index is a hypothesis like any other (the model pins it)
            if (!orbx_set_ok<3>(P.sets + 3 * (size_t)i, P.n, false)) { *why = "set index outside [0, n)"; return ORBX_BAD_ARGUMENT; }
        if (!sim3_add(w, P).ok) { *why = "too many iterations or correspondences for 32-bit offsets"; return ORBX_UNSUPPORTED; }
    }
    plan = w.plan(nproblems, sizeof(DSim3Prob), sizeof(OrbxSim3Hyp));
    return ORBX_OK;
}

void orbx_sim3_pack(const orbx_sim3_problem *problems, const OrbxSim3Plan &plan, uint8_t *dst) {
    if (plan.nlaunch <= 0) return;
    DSim3Prob *dp = (DSim3Prob *)(dst + plan.o_prob);
    int32_t *sets = (int32_t *)(dst + plan.o_sets);
    float *pts = (float *)(dst + plan.o_pts);
    OrbxRansacWalk w = sim3_walk((int32_t *)(dst + plan.o_hyp_prob), (int32_t *)(dst + plan.o_groups));
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_sim3_problem &P = problems[k];
        if (!sim3_launches(P)) continue;
        const OrbxRansacWalk::At at = sim3_add(w, P);
        DSim3Prob &D = dp[at.j];
        D.n = P.n; D.iterations = P.iterations; D.fix_scale = P.fix_scale ? 1 : 0; D.nwords = at.nwords;
        D.iter_off = at.hyp_off; D.pts_off = at.pts_off; D.word_off = at.word_off; D.pad = 0;
        memcpy(D.K1, P.camera1, sizeof(D.K1));
        memcpy(D.K2, P.camera2, sizeof(D.K2));
        memcpy(sets + 3 * (size_t)at.hyp_off, P.sets, (size_t)P.iterations * 3 * sizeof(int32_t));
        float *pl = pts + at.pts_off;
        const size_t n = (size_t)P.n;
        for (size_t i = 0; i < n; ++i) {
            for (int c = 0; c < 3; ++c) { pl[c * n + i] = P.x1c[3 * i + c]; pl[(3 + c) * n + i] = P.x2c[3 * i + c]; }
            pl[6 * n + i] = P.max_err1[i];
            pl[7 * n + i] = P.max_err2[i];
            // mvP1im1, mvP2im2: FromCameraToImage of the solver's constructor
            orbx_sim3_to_image(P.x1c[3 * i], P.x1c[3 * i + 1], P.x1c[3 * i + 2], P.camera1, &pl[8 * n + i], &pl[9 * n + i]);
            orbx_sim3_to_image(P.x2c[3 * i], P.x2c[3 * i + 1], P.x2c[3 * i + 2], P.camera2, &pl[10 * n + i], &pl[11 * n + i]);
        }
    }
}

void orbx_sim3_host_run(const OrbxSim3Plan &plan, const uint8_t *in, uint8_t *out) {
    const DSim3Prob *dp = (const DSim3Prob *)(in + plan.o_prob);
    const int32_t *sets = (const int32_t *)(in + plan.o_sets);
    const float *pts = (const float *)(in + plan.o_pts);
    OrbxSim3Hyp *hyp = (OrbxSim3Hyp *)(out + plan.o_hyp);
    uint64_t *masks = (uint64_t *)(out + plan.o_masks);
    int32_t *counts = (int32_t *)(out + plan.o_tally);
    for (int j = 0; j < plan.nlaunch; ++j) {
        const DSim3Prob &D = dp[j];
        const size_t n = (size_t)D.n;
        const float *pl = pts + D.pts_off;
        for (int i = 0; i < D.iterations; ++i) {
            const size_t h = (size_t)D.iter_off + i;
            float P1[9], P2[9];
            for (int c = 0; c < 3; ++c) {
                const size_t idx = (size_t)sets[3 * h + c];
                for (int r = 0; r < 3; ++r) { P1[3 * c + r] = pl[r * n + idx]; P2[3 * c + r] = pl[(3 + r) * n + idx]; }
            }
            OrbxSim3Hyp H;
            orbx_sim3_compute(P1, P2, D.fix_scale, H);
            hyp[h] = H;
            int cnt = 0;
            uint64_t *mw = masks + (size_t)D.word_off + (size_t)i * D.nwords;
            for (int w = 0; w < D.nwords; ++w) {
                uint64_t word = 0;
                for (int b = 0; b < 64; ++b) {
                    const size_t p = (size_t)w * 64 + b;
                    if (p >= n) break;
                    const float x1[3] = {pl[p], pl[n + p], pl[2 * n + p]}, x2[3] = {pl[3 * n + p], pl[4 * n + p], pl[5 * n + p]};
                    const float p1[2] = {pl[8 * n + p], pl[9 * n + p]}, p2[2] = {pl[10 * n + p], pl[11 * n + p]};
                    if (orbx_sim3_inlier(H.T12, H.T21, D.K1, D.K2, x1, x2, p1, p2, pl[6 * n + p], pl[7 * n + p])) { word |= (uint64_t)1 << b; ++cnt; }
                }
                mw[w] = word;
            }
            counts[h] = cnt;
        }
    }
}

orbx_sim3_batch *orbx_sim3_batch_new(const orbx_sim3_problem *problems, const OrbxSim3Plan &plan) {
    orbx_sim3_batch *b = new orbx_sim3_batch();
    b->st.resize((size_t)plan.nproblems);
    b->o_hyp = plan.o_hyp; b->o_masks = plan.o_masks; b->o_counts = plan.o_tally;
    OrbxRansacWalk w = sim3_walk();
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_sim3_problem &P = problems[k];
        OrbxSim3State &S = b->st[k];
        S.n = P.n; S.min_inliers = P.min_inliers; S.iterations = P.iterations; S.nwords = (P.n + 63) / 64;
        if (!sim3_launches(P)) continue;
        const OrbxRansacWalk::At at = sim3_add(w, P);
        S.iter_off = at.hyp_off; S.word_off = (size_t)at.word_off;
    }
    b->out.assign(plan.nlaunch > 0 ? plan.out_bytes : 0, 0);
    return b;
}

void orbx_sim3_batch_take(orbx_sim3_batch *b, const OrbxSim3Plan &plan, const uint8_t *out) { memcpy(b->out.data(), out, plan.out_bytes); }

int32_t orbx_sim3_cursor_iterate(orbx_sim3_batch *b, int k, int n_iterations, int32_t *no_more, uint8_t *inliers, int32_t *ninliers,
                                 float *T12, const char **why) {
    OrbxSim3State *cs = orbx_batch_state(b, k, why);
    if (!cs) return -1;
    if (!no_more || !ninliers || !T12 || (cs->n > 0 && !inliers)) { *why = "null result pointer"; return -1; }
    OrbxSim3State &S = *cs;
    *no_more = 0;                                              // bNoMore = false; vbInliers all false; nInliers = 0
    if (S.n > 0) memset(inliers, 0, (size_t)S.n);
    *ninliers = 0;
    if (S.n < S.min_inliers) { *no_more = 1; return 0; }
    const int32_t *counts = (const int32_t *)(b->out.data() + b->o_counts) + S.iter_off;
    int cur = 0;
    while (S.done < S.iterations && cur < n_iterations) {
        ++cur;
        const int i = S.done++;
        if (counts[i] >= S.best_inliers) {
            S.best_inliers = counts[i];
            S.best_it = i;
            if (counts[i] > S.min_inliers) {
                *ninliers = counts[i];
                const uint64_t *mw = (const uint64_t *)(b->out.data() + b->o_masks) + S.word_off + (size_t)i * S.nwords;
                orbx_unpack_mask(mw, S.n, inliers);
                memcpy(T12, ((const OrbxSim3Hyp *)(b->out.data() + b->o_hyp))[S.iter_off + i].T12, 16 * sizeof(float));
                return 1;
            }
        }
    }
    if (S.done >= S.iterations) *no_more = 1;
    return 0;
}

orbx_status orbx_sim3_cursor_best(const orbx_sim3_batch *b, int k, float *R, float *t, float *s, const char **why) {
    const OrbxSim3State *S = orbx_batch_state(b, k, why);
    if (!S) return ORBX_BAD_ARGUMENT;
    if (!R || !t || !s) { *why = "null result pointer"; return ORBX_BAD_ARGUMENT; }
    if (S->best_it < 0) { *why = "no iteration of this solver has run"; return ORBX_BAD_ARGUMENT; }
    const OrbxSim3Hyp &H = ((const OrbxSim3Hyp *)(b->out.data() + b->o_hyp))[S->iter_off + S->best_it];
    memcpy(R, H.R, sizeof(H.R));
    memcpy(t, H.t, sizeof(H.t));
    *s = H.s;
    return ORBX_OK;
}

orbx_status orbx_sim3_cursor_counts(const orbx_sim3_batch *b, int k, int32_t *counts, int32_t *niterations, const char **why) {
    const OrbxSim3State *S = orbx_batch_state(b, k, why);
    if (!S) return ORBX_BAD_ARGUMENT;
    const int nit = S->iter_off < 0 ? 0 : S->iterations;
    if (nit > 0 && !counts) { *why = "null counts"; return ORBX_BAD_ARGUMENT; }
    if (nit > 0) memcpy(counts, (const int32_t *)(b->out.data() + b->o_counts) + S->iter_off, (size_t)nit * sizeof(int32_t));
    if (niterations) *niterations = nit;
    return ORBX_OK;
}

orbx_status orbx_sim3_cursor_hypothesis(const orbx_sim3_batch *b, int k, int iteration, float *hyp48, uint64_t *mask_words,
                                        const char **why) {
    const OrbxSim3State *S = orbx_batch_state(b, k, why);
    if (!S) return ORBX_BAD_ARGUMENT;
    if (S->iter_off < 0 || iteration < 0 || iteration >= S->iterations) { *why = "iteration outside the solver's stored results"; return ORBX_BAD_ARGUMENT; }
    if (hyp48) memcpy(hyp48, (const OrbxSim3Hyp *)(b->out.data() + b->o_hyp) + S->iter_off + iteration, sizeof(OrbxSim3Hyp));
    if (mask_words && S->nwords > 0)
        memcpy(mask_words, (const uint64_t *)(b->out.data() + b->o_masks) + S->word_off + (size_t)iteration * S->nwords,
               (size_t)S->nwords * sizeof(uint64_t));
    return ORBX_OK;
}

// Sim3Solver::SetRansacParameters (:153-191): what mRansacMaxIts becomes
extern "C" int32_t orbx_sim3_ransac_iterations(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations) {
    const float epsilon = (float)min_inliers / n;              // float epsilon = (float)mRansacMinInliers/N
    int nIterations;
    if (min_inliers == n) nIterations = 1;
    else {
        // outside int's range when epsilon^3 rounds to 0 or exceeds 1: NaN and +inf then count as "more than max_iterations"
        nIterations = orbx_to_int_clamped(std::ceil(std::log(1 - probability) / std::log(1 - std::pow(epsilon, 3))));
    }
    return std::max(1, std::min(nIterations, max_iterations));
}

extern "C" double orbx_sim3_atan2(double y, double x) { return orbx_sim3_atan2_pos(y, x); }
