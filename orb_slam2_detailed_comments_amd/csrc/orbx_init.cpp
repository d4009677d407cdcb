// orbx_init.cpp -- host side of the batched Initializer H / F RANSAC (orbx_init.h): validation of a call, Normalize, the packing
// of all problems into one staging block, the library's host path -- the header's scalar code compiled by the host compiler over
// that same block -- and the result object with its accessors.  HIP-free.  The entry points (orbx_map_batches.cpp) own the
// staging block, the arena and the launches.
#include <cmath>
#include <cstring>
#include <algorithm>
#include "orbx_init.h"

static inline int init_nmodels(int32_t models) { return (models & 1) + ((models >> 1) & 1); }
static inline bool init_launches(const orbx_init_problem &P) { return orbx_init_launches(P); }
static inline OrbxRansacWalk init_walk(int32_t *hyp_prob = nullptr, int32_t *groups = nullptr) {
    return OrbxRansacWalk(0x0fffffff, 0x3fffffff, hyp_prob, groups);
}
static inline OrbxRansacWalk::At init_add(OrbxRansacWalk &w, int32_t n, int32_t iterations, int32_t models) {
    return w.add(n, (size_t)iterations * init_nmodels(models), (size_t)iterations * 8, ORBX_INIT_PLANES, ORBX_INIT_SCORE_LANES);
}

orbx_status orbx_init_plan(int nproblems, const orbx_init_problem *problems, OrbxInitPlan &plan, const char **why) {
    plan = OrbxInitPlan();
    if (nproblems < 0) { *why = "nproblems < 0"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !problems) { *why = "null problem array"; return ORBX_BAD_ARGUMENT; }
    OrbxRansacWalk w = init_walk();
    for (int k = 0; k < nproblems; ++k) {
        const orbx_init_problem &P = problems[k];
        if (P.n1 < 0 || P.n2 < 0 || P.n < 0) { *why = "a negative count"; return ORBX_BAD_ARGUMENT; }
        if ((P.n1 > 0 && !P.keys1) || (P.n2 > 0 && !P.keys2)) { *why = "null keypoint array of positive size"; return ORBX_BAD_ARGUMENT; }
        if (P.n > 0 && !P.matches) { *why = "null match array with n > 0"; return ORBX_BAD_ARGUMENT; }
        if (P.iterations < 1) { *why = "iterations < 1"; return ORBX_BAD_ARGUMENT; }
        if (!std::isfinite(P.sigma) || !(P.sigma > 0.0f)) { *why = "sigma is not finite or not > 0"; return ORBX_BAD_ARGUMENT; }
        if (P.models & ~(ORBX_INIT_H | ORBX_INIT_F)) { *why = "models has a bit outside ORBX_INIT_H | ORBX_INIT_F"; return ORBX_BAD_ARGUMENT; }
        for (int i = 0; i < P.n; ++i) {
            const int32_t a = P.matches[2 * (size_t)i], b = P.matches[2 * (size_t)i + 1];
            if (a < 0 || a >= P.n1 || b < 0 || b >= P.n2) { *why = "a match index outside its frame"; return ORBX_BAD_ARGUMENT; }
        }
        if (!init_launches(P)) continue;
        if (!P.sets) { *why = "null sets"; return ORBX_BAD_ARGUMENT; }
        for (int i = 0; i < P.iterations; ++i)
            if (!orbx_set_ok<8>(P.sets + 8 * (size_t)i, P.n, true)) { *why = "set index outside [0, n) or repeated within its set"; return ORBX_BAD_ARGUMENT; }
        if (!init_add(w, P.n, P.iterations, P.models).ok) { *why = "too many iterations or matches for 32-bit offsets"; return ORBX_UNSUPPORTED; }
    }
    plan = w.plan(nproblems, sizeof(DInitProb), sizeof(OrbxInitHyp));
    return ORBX_OK;
}

// Normalize (:1549-1617) over ALL N keypoints of a frame: the four float sums in index order, the mean as sum / (float)N,
// sX = 1.0 / meanDevX rounded to float (the correctly rounded float division, see orbx_init.h).  mean_scale = meanX, meanY, sX, sY.
static void init_normalize(const float *keys, int32_t N, float *T, float *mean_scale) {
    float meanX = 0, meanY = 0;
    for (int32_t i = 0; i < N; ++i) {
        meanX = meanX + keys[2 * (size_t)i];
        meanY = meanY + keys[2 * (size_t)i + 1];
    }
    meanX = meanX / (float)N;
    meanY = meanY / (float)N;
    float meanDevX = 0, meanDevY = 0;
    for (int32_t i = 0; i < N; ++i) {
        meanDevX = meanDevX + std::fabs(keys[2 * (size_t)i] - meanX);
        meanDevY = meanDevY + std::fabs(keys[2 * (size_t)i + 1] - meanY);
    }
    meanDevX = meanDevX / (float)N;
    meanDevY = meanDevY / (float)N;
    const float sX = 1.0f / meanDevX, sY = 1.0f / meanDevY;
    for (int i = 0; i < 9; ++i) T[i] = i % 4 == 0 ? 1.0f : 0.0f;
    T[0] = sX;
    T[4] = sY;
    T[2] = orbx_canonf(-meanX * sX);
    T[5] = orbx_canonf(-meanY * sY);
    T[0] = orbx_canonf(T[0]);
    T[4] = orbx_canonf(T[4]);
    mean_scale[0] = meanX; mean_scale[1] = meanY; mean_scale[2] = sX; mean_scale[3] = sY;
}

void orbx_init_pack(const orbx_init_problem *problems, const OrbxInitPlan &plan, uint8_t *dst) {
    if (plan.nlaunch <= 0) return;
    DInitProb *dp = (DInitProb *)(dst + plan.o_prob);
    int32_t *sets = (int32_t *)(dst + plan.o_sets);
    float *pts = (float *)(dst + plan.o_pts);
    OrbxRansacWalk w = init_walk((int32_t *)(dst + plan.o_hyp_prob), (int32_t *)(dst + plan.o_groups));
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_init_problem &P = problems[k];
        if (!init_launches(P)) continue;
        const OrbxRansacWalk::At at = init_add(w, P.n, P.iterations, P.models);
        DInitProb &D = dp[at.j];
        D.n = P.n; D.iterations = P.iterations; D.nwords = at.nwords; D.models = P.models;
        D.hyp_off = at.hyp_off; D.pts_off = at.pts_off; D.word_off = at.word_off; D.set_off = at.set_off;
        float T2[9], ms1[4], ms2[4];
        init_normalize(P.keys1, P.n1, D.T1, ms1);
        init_normalize(P.keys2, P.n2, T2, ms2);
        orbx_init_inv3(T2, D.T2inv);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) D.T2t[3 * r + c] = T2[3 * c + r];
        for (int i = 0; i < 9; ++i) D.T2inv[i] = orbx_canonf(D.T2inv[i]);
        D.inv_sigma2 = orbx_init_inv_sigma2(P.sigma);
        memcpy(sets + at.set_off, P.sets, (size_t)P.iterations * 8 * sizeof(int32_t));
        float *pl = pts + at.pts_off;
        const size_t n = (size_t)P.n;
        for (size_t i = 0; i < n; ++i) {
            const float *a = P.keys1 + 2 * (size_t)P.matches[2 * i], *b = P.keys2 + 2 * (size_t)P.matches[2 * i + 1];
            pl[i] = (a[0] - ms1[0]) * ms1[2];                   // vPn1[first]: (x - meanX) * sX
            pl[n + i] = (a[1] - ms1[1]) * ms1[3];
            pl[2 * n + i] = (b[0] - ms2[0]) * ms2[2];
            pl[3 * n + i] = (b[1] - ms2[1]) * ms2[3];
            pl[4 * n + i] = a[0]; pl[5 * n + i] = a[1]; pl[6 * n + i] = b[0]; pl[7 * n + i] = b[1];
        }
    }
}

void orbx_init_host_run(const OrbxInitPlan &plan, const uint8_t *in, uint8_t *out) {
    const DInitProb *dp = (const DInitProb *)(in + plan.o_prob);
    const int32_t *sets = (const int32_t *)(in + plan.o_sets);
    const float *pts = (const float *)(in + plan.o_pts);
    OrbxInitHyp *hyp = (OrbxInitHyp *)(out + plan.o_hyp);
    uint64_t *masks = (uint64_t *)(out + plan.o_masks);
    float *scores = (float *)(out + plan.o_tally);
    float ws[ORBX_INIT_WS_FLOATS];
    const OrbxInitWs W = {ws, 1};
    for (int j = 0; j < plan.nlaunch; ++j) {
        const DInitProb &D = dp[j];
        const float *pl = pts + D.pts_off;
        const size_t n = (size_t)D.n;
        const int nh = orbx_init_nhyp(D);
        for (int l = 0; l < nh; ++l) {
            const bool is_h = orbx_init_is_h(D, l);
            const int32_t *s = sets + D.set_off + 8 * (size_t)orbx_init_iteration(D, l);
            for (int c = 0; c < 8; ++c)
                for (int r = 0; r < 4; ++r) W(ORBX_INIT_PTS + 4 * c + r) = pl[r * n + (size_t)s[c]];
            OrbxInitHyp &H = hyp[(size_t)D.hyp_off + l];
            orbx_init_hypothesis(W, is_h, D.T1, is_h ? D.T2inv : D.T2t, H);
            uint64_t *mw = masks + (size_t)D.word_off + (size_t)l * D.nwords;
            float score = 0.0f;
            uint64_t word = 0;
            for (size_t m = 0; m < n; ++m) {
                const float u1 = pl[4 * n + m], v1 = pl[5 * n + m], u2 = pl[6 * n + m], v2 = pl[7 * n + m];
                const bool in = is_h ? orbx_init_check_h(H.M, H.Minv, u1, v1, u2, v2, D.inv_sigma2, score)
                                     : orbx_init_check_f(H.M, u1, v1, u2, v2, D.inv_sigma2, score);
                if (in) word |= (uint64_t)1 << (m & 63);
                if ((m & 63) == 63 || m + 1 == n) { mw[m >> 6] = word; word = 0; }
            }
            scores[(size_t)D.hyp_off + l] = orbx_canonf(score);
        }
    }
}

orbx_init_batch *orbx_init_batch_new(const orbx_init_problem *problems, const OrbxInitPlan &plan) {
    orbx_init_batch *b = new orbx_init_batch();
    b->st.resize((size_t)plan.nproblems);
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_init_problem &P = problems[k];
        OrbxInitResult &S = b->st[k];
        S.n = P.n; S.iterations = P.iterations; S.nwords = (P.n + 63) / 64; S.models = P.models;
        S.launches = init_launches(P);
        float ms[4];
        init_normalize(P.keys1, P.n1, S.T1, ms);
        init_normalize(P.keys2, P.n2, S.T2, ms);
        S.RH = orbx_canonf(S.SH / (S.SH + S.SF));          // 0 / 0 until results arrive
    }
    return b;
}

// score = 0; if (currentScore > score) ...: the first strict maximum; -1 when no iteration scored above 0 (a NaN never does)
static int32_t init_best(const float *s, int n, float *best) {
    float score = 0.0f;
    int32_t it = -1;
    for (int i = 0; i < n; ++i)
        if (s[i] > score) { score = s[i]; it = i; }
    *best = score;
    return it;
}

void orbx_init_batch_take(orbx_init_batch *b, const OrbxInitPlan &plan, const uint8_t *out) {
    const OrbxInitHyp *hyp = (const OrbxInitHyp *)(out + plan.o_hyp);
    const uint64_t *masks = (const uint64_t *)(out + plan.o_masks);
    const float *scores = (const float *)(out + plan.o_tally);
    OrbxRansacWalk w = init_walk();
    for (OrbxInitResult &S : b->st) {
        if (!S.launches) continue;
        const OrbxRansacWalk::At at = init_add(w, S.n, S.iterations, S.models);
        const size_t nh = (size_t)S.iterations * init_nmodels(S.models), nw = nh * (size_t)S.nwords;
        S.hyp.assign(hyp + at.hyp_off, hyp + at.hyp_off + nh);
        S.scores.assign(scores + at.hyp_off, scores + at.hyp_off + nh);
        S.masks.assign(masks + at.word_off, masks + at.word_off + nw);
        const int fo = (S.models & ORBX_INIT_H) ? S.iterations : 0;
        if (S.models & ORBX_INIT_H) S.itH = init_best(S.scores.data(), S.iterations, &S.SH);
        if (S.models & ORBX_INIT_F) S.itF = init_best(S.scores.data() + fo, S.iterations, &S.SF);
        S.RH = orbx_canonf(S.SH / (S.SH + S.SF));          // float RH = SH / (SH + SF)
        if (S.itH < 0 && S.itF < 0) S.model = ORBX_INIT_NONE;
        else S.model = ((double)S.RH > 0.40) ? ORBX_INIT_H : ORBX_INIT_F;   // the float promoted against the double constant
    }
}

// first hypothesis of `model` in the problem's stored results, or -1 when the model has none
static int init_model_off(const OrbxInitResult &S, int model) {
    if (!S.launches || !(S.models & model)) return -1;
    return model == ORBX_INIT_F && (S.models & ORBX_INIT_H) ? S.iterations : 0;
}
static void init_unpack(const OrbxInitResult &S, int off, int it, uint8_t *inliers) {
    if (!inliers) return;
    if (it < 0) { if (S.n > 0) memset(inliers, 0, (size_t)S.n); return; }
    orbx_unpack_mask(S.masks.data() + (size_t)(off + it) * S.nwords, S.n, inliers);
}

orbx_status orbx_init_get_result(const orbx_init_batch *b, int k, float *SH, float *SF, float *H21, float *F21, uint8_t *inliersH,
                                 uint8_t *inliersF, int32_t *itH, int32_t *itF, float *RH, int32_t *model, const char **why) {
    const OrbxInitResult *S = orbx_batch_state(b, k, why);
    if (!S) return ORBX_BAD_ARGUMENT;
    const int oh = init_model_off(*S, ORBX_INIT_H), of = init_model_off(*S, ORBX_INIT_F);
    if (SH) *SH = S->SH;
    if (SF) *SF = S->SF;
    if (H21) { if (S->itH >= 0) memcpy(H21, S->hyp[oh + S->itH].M, 9 * sizeof(float)); else memset(H21, 0, 9 * sizeof(float)); }
    if (F21) { if (S->itF >= 0) memcpy(F21, S->hyp[of + S->itF].M, 9 * sizeof(float)); else memset(F21, 0, 9 * sizeof(float)); }
    init_unpack(*S, oh, S->itH, inliersH);
    init_unpack(*S, of, S->itF, inliersF);
    if (itH) *itH = S->itH;
    if (itF) *itF = S->itF;
    if (RH) *RH = S->RH;
    if (model) *model = S->model;
    return ORBX_OK;
}

static bool init_model_ok(int model, const char **why) {
    if (model == ORBX_INIT_H || model == ORBX_INIT_F) return true;
    *why = "model is neither ORBX_INIT_H nor ORBX_INIT_F";
    return false;
}

orbx_status orbx_init_get_scores(const orbx_init_batch *b, int k, int model, float *scores, int32_t *niterations, const char **why) {
    const OrbxInitResult *S = orbx_batch_state(b, k, why);
    if (!S || !init_model_ok(model, why)) return ORBX_BAD_ARGUMENT;
    const int off = init_model_off(*S, model);
    if (scores && off >= 0) memcpy(scores, S->scores.data() + off, (size_t)S->iterations * sizeof(float));
    if (niterations) *niterations = off >= 0 ? S->iterations : 0;
    return ORBX_OK;
}

orbx_status orbx_init_get_hypothesis(const orbx_init_batch *b, int k, int model, int iteration, float *M9, float *Minv9, float *score,
                                     uint64_t *mask_words, const char **why) {
    const OrbxInitResult *S = orbx_batch_state(b, k, why);
    if (!S || !init_model_ok(model, why)) return ORBX_BAD_ARGUMENT;
    const int off = init_model_off(*S, model);
    if (off < 0 || iteration < 0 || iteration >= S->iterations) { *why = "iteration outside the problem's stored results"; return ORBX_BAD_ARGUMENT; }
    const OrbxInitHyp &H = S->hyp[off + iteration];
    if (M9) memcpy(M9, H.M, sizeof(H.M));
    if (Minv9) memcpy(Minv9, H.Minv, sizeof(H.Minv));
    if (score) *score = S->scores[off + iteration];
    if (mask_words && S->nwords > 0)
        memcpy(mask_words, S->masks.data() + (size_t)(off + iteration) * S->nwords, (size_t)S->nwords * sizeof(uint64_t));
    return ORBX_OK;
}

orbx_status orbx_init_get_normalization(const orbx_init_batch *b, int k, float *T1, float *T2, const char **why) {
    const OrbxInitResult *S = orbx_batch_state(b, k, why);
    if (!S) return ORBX_BAD_ARGUMENT;
    if (T1) memcpy(T1, S->T1, sizeof(S->T1));
    if (T2) memcpy(T2, S->T2, sizeof(S->T2));
    return ORBX_OK;
}
