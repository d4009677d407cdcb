// orbx_pnp.cpp -- host side of the batched PnPsolver RANSAC (orbx_pnp.h): validation of a call, the packing of all problems into
// one staging block, the library's host path -- the header's scalar code compiled by the host compiler over that same block --
// SetRansacParameters, Refine, and the iterate() cursor over the stored results.  HIP-free.  The entry points
// (orbx_map_batches.cpp) own the staging block, the arena and the launches.
#include <cmath>
#include <cstring>
#include <algorithm>
#include "orbx_pnp.h"

static inline bool pnp_launches(const orbx_pnp_problem &P) { return P.n >= P.min_inliers; }
static inline bool pnp_set_ok(const int32_t *s, int32_t n) { return orbx_set_ok<4>(s, n, true); }
static inline OrbxRansacWalk pnp_walk(int32_t *hyp_prob = nullptr, int32_t *groups = nullptr) {
    return OrbxRansacWalk(0x0fffffff, 0x3fffffff, hyp_prob, groups);
}
static inline OrbxRansacWalk::At pnp_add(OrbxRansacWalk &w, int32_t n, int32_t iterations) {
    return w.add(n, (size_t)iterations, (size_t)iterations * 4, ORBX_PNP_PLANES, ORBX_PNP_WAVES);
}

orbx_status orbx_pnp_plan(int nproblems, const orbx_pnp_problem *problems, OrbxPnpPlan &plan, const char **why) {
    plan = OrbxPnpPlan();
    if (nproblems < 0) { *why = "nproblems < 0"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !problems) { *why = "null problem array"; return ORBX_BAD_ARGUMENT; }
    OrbxRansacWalk w = pnp_walk();
    for (int k = 0; k < nproblems; ++k) {
        const orbx_pnp_problem &P = problems[k];
        if (P.n < 0) { *why = "n < 0"; return ORBX_BAD_ARGUMENT; }
        if (P.iterations < 1) { *why = "iterations < 1"; return ORBX_BAD_ARGUMENT; }
        if (P.n > 0 && (!P.p3dw || !P.p2d || !P.max_err)) { *why = "null correspondence array with n > 0"; return ORBX_BAD_ARGUMENT; }
        if (!pnp_launches(P)) continue;
        if (!P.sets) { *why = "null sets"; return ORBX_BAD_ARGUMENT; }
        for (int i = 0; i < P.iterations; ++i)
            if (!pnp_set_ok(P.sets + 4 * (size_t)i, P.n)) { *why = "set index outside [0, n) or repeated within its set"; return ORBX_BAD_ARGUMENT; }
        if (!pnp_add(w, P.n, P.iterations).ok) { *why = "too many iterations or correspondences for 32-bit offsets"; return ORBX_UNSUPPORTED; }
    }
    plan = w.plan(nproblems, sizeof(DPnpProb), sizeof(OrbxPnpHyp));
    return ORBX_OK;
}

static void pnp_planes(const orbx_pnp_problem &P, float *pl) {
    const size_t n = (size_t)P.n;
    for (size_t i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) pl[c * n + i] = P.p3dw[3 * i + c];
        pl[3 * n + i] = P.p2d[2 * i];
        pl[4 * n + i] = P.p2d[2 * i + 1];
        pl[5 * n + i] = P.max_err[i];
    }
}

void orbx_pnp_pack(const orbx_pnp_problem *problems, const OrbxPnpPlan &plan, uint8_t *dst) {
    if (plan.nlaunch <= 0) return;
    DPnpProb *dp = (DPnpProb *)(dst + plan.o_prob);
    int32_t *sets = (int32_t *)(dst + plan.o_sets);
    float *pts = (float *)(dst + plan.o_pts);
    OrbxRansacWalk w = pnp_walk((int32_t *)(dst + plan.o_hyp_prob), (int32_t *)(dst + plan.o_groups));
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_pnp_problem &P = problems[k];
        if (!pnp_launches(P)) continue;
        const OrbxRansacWalk::At at = pnp_add(w, P.n, P.iterations);
        DPnpProb &D = dp[at.j];
        D.n = P.n; D.iterations = P.iterations; D.nwords = at.nwords; D.pad = 0;
        D.iter_off = at.hyp_off; D.pts_off = at.pts_off; D.word_off = at.word_off; D.pad2 = 0;
        memcpy(D.cam, P.camera, sizeof(D.cam));
        memcpy(sets + at.set_off, P.sets, (size_t)P.iterations * 4 * sizeof(int32_t));
        pnp_planes(P, pts + at.pts_off);
    }
}

// compute_pose on the correspondences idx[0 .. m) of the planes, then CheckInliers over all n: one iteration, or Refine
static void pnp_evaluate(const float *pl, size_t n, const double *cam, const int32_t *idx, int m, std::vector<double> &ws,
                         OrbxPnpHyp &H, uint64_t *mw, int nwords, int32_t *count) {
    ws.resize((size_t)ORBX_PNP_WS_DOUBLES(m));
    const OrbxPnpWs W = {ws.data(), 1};
    for (int c = 0; c < m; ++c) {
        const size_t i = (size_t)idx[c];
        for (int r = 0; r < 3; ++r) W(ORBX_PNP_FIXED + 3 * c + r) = (double)pl[r * n + i];
        W(ORBX_PNP_FIXED + 3 * m + 2 * c) = (double)pl[3 * n + i];
        W(ORBX_PNP_FIXED + 3 * m + 2 * c + 1) = (double)pl[4 * n + i];
    }
    double Rt[12];
    const int N = orbx_pnp_compute_pose(W, m, cam, Rt);
    orbx_pnp_store(Rt, N, H);
    int cnt = 0;
    for (int w = 0; w < nwords; ++w) {
        uint64_t word = 0;
        for (int b = 0; b < 64; ++b) {
            const size_t p = (size_t)w * 64 + b;
            if (p >= n) break;
            if (orbx_pnp_inlier(H.R, H.t, cam, pl[p], pl[n + p], pl[2 * n + p], pl[3 * n + p], pl[4 * n + p], pl[5 * n + p])) {
                word |= (uint64_t)1 << b;
                ++cnt;
            }
        }
        mw[w] = word;
    }
    *count = cnt;
}

void orbx_pnp_host_run(const OrbxPnpPlan &plan, const uint8_t *in, uint8_t *out) {
    const DPnpProb *dp = (const DPnpProb *)(in + plan.o_prob);
    const int32_t *sets = (const int32_t *)(in + plan.o_sets);
    const float *pts = (const float *)(in + plan.o_pts);
    OrbxPnpHyp *hyp = (OrbxPnpHyp *)(out + plan.o_hyp);
    uint64_t *masks = (uint64_t *)(out + plan.o_masks);
    int32_t *counts = (int32_t *)(out + plan.o_tally);
    std::vector<double> ws;
    for (int j = 0; j < plan.nlaunch; ++j) {
        const DPnpProb &D = dp[j];
        for (int i = 0; i < D.iterations; ++i) {
            const size_t h = (size_t)D.iter_off + i;
            pnp_evaluate(pts + D.pts_off, (size_t)D.n, D.cam, sets + 4 * h, 4, ws, hyp[h],
                         masks + (size_t)D.word_off + (size_t)i * D.nwords, D.nwords, &counts[h]);
        }
    }
}

orbx_pnp_batch *orbx_pnp_batch_new(const orbx_pnp_problem *problems, const OrbxPnpPlan &plan) {
    orbx_pnp_batch *b = new orbx_pnp_batch();
    b->st.resize((size_t)plan.nproblems);
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_pnp_problem &P = problems[k];
        OrbxPnpSolver &S = b->st[k];
        S.n = P.n; S.min_inliers = P.min_inliers; S.max_its = P.iterations; S.nwords = (P.n + 63) / 64;
        S.launches = pnp_launches(P);
        memcpy(S.cam, P.camera, sizeof(S.cam));
        if (!S.launches) continue;
        S.planes.resize((size_t)P.n * ORBX_PNP_PLANES);
        pnp_planes(P, S.planes.data());
    }
    return b;
}

void orbx_pnp_batch_take(orbx_pnp_batch *b, const OrbxPnpPlan &plan, const uint8_t *out) {
    const OrbxPnpHyp *hyp = (const OrbxPnpHyp *)(out + plan.o_hyp);
    const uint64_t *masks = (const uint64_t *)(out + plan.o_masks);
    const int32_t *counts = (const int32_t *)(out + plan.o_tally);
    OrbxRansacWalk w = pnp_walk();
    for (OrbxPnpSolver &S : b->st) {
        if (!S.launches) continue;
        const OrbxRansacWalk::At at = pnp_add(w, S.n, S.max_its);
        const size_t ni = (size_t)S.max_its, nw = ni * (size_t)S.nwords;
        S.hyp.assign(hyp + at.hyp_off, hyp + at.hyp_off + ni);
        S.counts.assign(counts + at.hyp_off, counts + at.hyp_off + ni);
        S.masks.assign(masks + at.word_off, masks + at.word_off + nw);
    }
}

// Refine (:386-438) of the best mask, computed when first asked for and kept while the best does not move
static const OrbxPnpRefined &pnp_refine(OrbxPnpSolver &S) {
    if (S.refined_it == S.best_it) return S.refined;
    const uint64_t *mw = S.masks.data() + (size_t)S.best_it * S.nwords;
    std::vector<int32_t> idx;
    for (int p = 0; p < S.n; ++p)
        if ((mw[p >> 6] >> (p & 63)) & 1u) idx.push_back(p);
    OrbxPnpRefined &R = S.refined;
    R.mask.assign((size_t)S.nwords, 0);
    std::vector<double> ws;
    pnp_evaluate(S.planes.data(), (size_t)S.n, S.cam, idx.data(), (int)idx.size(), ws, R.hyp, R.mask.data(), S.nwords, &R.count);
    R.ok = R.count > S.min_inliers;
    S.refined_it = S.best_it;
    return R;
}

int32_t orbx_pnp_cursor_iterate(orbx_pnp_batch *b, int k, int n_iterations, int32_t *no_more, uint8_t *inliers, int32_t *ninliers,
                                float *Tcw, const char **why) {
    OrbxPnpSolver *cs = orbx_batch_state(b, k, why);
    if (!cs) return -1;
    if (!no_more || !ninliers || !Tcw || (cs->n > 0 && !inliers)) { *why = "null result pointer"; return -1; }
    OrbxPnpSolver &S = *cs;
    *no_more = 0;                                              // bNoMore = false; vbInliers empty; nInliers = 0
    if (S.n > 0) memset(inliers, 0, (size_t)S.n);
    *ninliers = 0;
    if (S.n < S.min_inliers) { *no_more = 1; return 0; }
    const int32_t done0 = S.done, best_inliers0 = S.best_inliers, best_it0 = S.best_it;
    int cur = 0;
    while (S.done < S.max_its || cur < n_iterations) {        // an OR, as in the source (:285)
        if ((size_t)S.done >= S.counts.size()) {               // past the stored iterations: nothing has happened
            S.done = done0; S.best_inliers = best_inliers0; S.best_it = best_it0;
            *why = "the replay needs an iteration past those stored: append sets and call again";
            return -2;
        }
        ++cur;
        const int i = S.done++;
        if (S.counts[i] >= S.min_inliers) {
            if (S.counts[i] > S.best_inliers) { S.best_inliers = S.counts[i]; S.best_it = i; }
            const OrbxPnpRefined &R = pnp_refine(S);
            if (R.ok) {
                *ninliers = R.count;
                orbx_unpack_mask(R.mask.data(), S.n, inliers);
                memcpy(Tcw, R.hyp.Tcw, 16 * sizeof(float));
                return 1;
            }
        }
    }
    if (S.done >= S.max_its) {
        *no_more = 1;
        if (S.best_inliers >= S.min_inliers) {
            *ninliers = S.best_inliers;
            orbx_unpack_mask(S.masks.data() + (size_t)S.best_it * S.nwords, S.n, inliers);
            memcpy(Tcw, S.hyp[S.best_it].Tcw, 16 * sizeof(float));
            return 1;
        }
    }
    return 0;
}

orbx_status orbx_pnp_cursor_append(orbx_pnp_batch *b, int k, int nsets, const int32_t *sets, const char **why) {
    OrbxPnpSolver *cs = orbx_batch_state(b, k, why);
    if (!cs) return ORBX_BAD_ARGUMENT;
    if (nsets < 0 || (nsets > 0 && !sets)) { *why = "nsets < 0 or null sets"; return ORBX_BAD_ARGUMENT; }
    OrbxPnpSolver &S = *cs;
    if (!S.launches) { *why = "a solver with n < min_inliers has no iterations"; return ORBX_BAD_ARGUMENT; }
    for (int i = 0; i < nsets; ++i)
        if (!pnp_set_ok(sets + 4 * (size_t)i, S.n)) { *why = "set index outside [0, n) or repeated within its set"; return ORBX_BAD_ARGUMENT; }
    std::vector<double> ws;
    for (int i = 0; i < nsets; ++i) {
        const size_t at = S.counts.size();
        S.hyp.emplace_back();
        S.counts.push_back(0);
        S.masks.resize((at + 1) * (size_t)S.nwords);
        pnp_evaluate(S.planes.data(), (size_t)S.n, S.cam, sets + 4 * (size_t)i, 4, ws, S.hyp[at], S.masks.data() + at * S.nwords,
                     S.nwords, &S.counts[at]);
    }
    return ORBX_OK;
}

orbx_status orbx_pnp_cursor_best(const orbx_pnp_batch *b, int k, float *Tcw, int32_t *ninliers, int32_t *iteration, const char **why) {
    const OrbxPnpSolver *S = orbx_batch_state(b, k, why);
    if (!S) return ORBX_BAD_ARGUMENT;
    if (S->best_it < 0) { *why = "no iteration of this solver has reached min_inliers"; return ORBX_BAD_ARGUMENT; }
    if (Tcw) memcpy(Tcw, S->hyp[S->best_it].Tcw, 16 * sizeof(float));
    if (ninliers) *ninliers = S->best_inliers;
    if (iteration) *iteration = S->best_it;
    return ORBX_OK;
}

orbx_status orbx_pnp_cursor_counts(const orbx_pnp_batch *b, int k, int32_t *counts, int32_t *niterations, const char **why) {
    const OrbxPnpSolver *S = orbx_batch_state(b, k, why);
    if (!S) return ORBX_BAD_ARGUMENT;
    if (counts && !S->counts.empty()) memcpy(counts, S->counts.data(), S->counts.size() * sizeof(int32_t));
    if (niterations) *niterations = (int32_t)S->counts.size();
    return ORBX_OK;
}

orbx_status orbx_pnp_cursor_hypothesis(const orbx_pnp_batch *b, int k, int iteration, double *Rt12, float *Tcw, int32_t *N,
                                       uint64_t *mask_words, const char **why) {
    const OrbxPnpSolver *S = orbx_batch_state(b, k, why);
    if (!S) return ORBX_BAD_ARGUMENT;
    if (iteration < 0 || (size_t)iteration >= S->counts.size()) { *why = "iteration outside the solver's stored results"; return ORBX_BAD_ARGUMENT; }
    const OrbxPnpHyp &H = S->hyp[iteration];
    if (Rt12) { memcpy(Rt12, H.R, sizeof(H.R)); memcpy(Rt12 + 9, H.t, sizeof(H.t)); }
    if (Tcw) memcpy(Tcw, H.Tcw, sizeof(H.Tcw));
    if (N) *N = H.N;
    if (mask_words && S->nwords > 0)
        memcpy(mask_words, S->masks.data() + (size_t)iteration * S->nwords, (size_t)S->nwords * sizeof(uint64_t));
    return ORBX_OK;
}

// PnPsolver::SetRansacParameters (:190-239): what mRansacMinInliers and mRansacMaxIts become for N = n
extern "C" void orbx_pnp_ransac_parameters(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations, int32_t min_set,
                                           float epsilon, int32_t *out_min_inliers, int32_t *out_iterations) {
    int nMinInliers = orbx_to_int_clamped((double)((float)n * epsilon));           // int nMinInliers = N*mRansacEpsilon
    if (nMinInliers < min_inliers) nMinInliers = min_inliers;
    if (nMinInliers < min_set) nMinInliers = min_set;
    if (epsilon < (float)nMinInliers / n) epsilon = (float)nMinInliers / n;
    int nIterations;
    if (nMinInliers == n) nIterations = 1;
    else nIterations = orbx_to_int_clamped(std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0))));
    if (out_min_inliers) *out_min_inliers = nMinInliers;
    if (out_iterations) *out_iterations = std::max(1, std::min(nIterations, max_iterations));
}
