// orbx_recon.cpp -- host side of the batched ReconstructH / ReconstructF (orbx_recon.h): validation of a call, the packing of all
// problems into one staging block, the library's host path -- the header's scalar code compiled by the host compiler over that
// same block --, acos and the accept / reject arithmetic of both functions, and the result object with its accessors.  HIP-free.
// The entry point (orbx_map_batches.cpp) owns the staging block, the arena and the launches.
#include <cmath>
#include <cstring>
#include <algorithm>
#include "orbx_recon.h"

static inline bool recon_launches(const orbx_recon_problem &P, int32_t *N = nullptr) {
    int32_t c = 0;
    for (int i = 0; i < P.n; ++i) c += P.inliers[i] ? 1 : 0;
    if (N) *N = c;
    return c > 0;
}
static inline int recon_nhyp(int model) { return model == ORBX_INIT_H ? 8 : 4; }
static const char *recon_camera_why(const float *K, float min_parallax) {
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(K[i])) return "an intrinsic is not finite";
    if (!(K[0] > 0.0f) || !(K[1] > 0.0f)) return "fx or fy is not > 0";
    if (std::isnan(min_parallax)) return "min_parallax is NaN";
    return nullptr;
}
// the per-hypothesis planes take 8 n matches of 3 floats: the 32-bit limit of a call
static inline bool recon_fits(size_t total_m) { return total_m <= (size_t)0x03ffffff; }

orbx_status orbx_recon_plan(int nproblems, const orbx_recon_problem *problems, OrbxReconPlan &plan, const char **why) {
    plan = OrbxReconPlan();
    if (nproblems < 0) { *why = "nproblems < 0"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !problems) { *why = "null problem array"; return ORBX_BAD_ARGUMENT; }
    plan.nproblems = nproblems;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_recon_problem &P = problems[k];
        if (P.n1 < 0 || P.n2 < 0 || P.n < 0) { *why = "a negative count"; return ORBX_BAD_ARGUMENT; }
        if ((P.n1 > 0 && !P.keys1) || (P.n2 > 0 && !P.keys2)) { *why = "null keypoint array of positive size"; return ORBX_BAD_ARGUMENT; }
        if (P.n > 0 && !P.matches) { *why = "null match array with n > 0"; return ORBX_BAD_ARGUMENT; }
        if (P.n > 0 && !P.inliers) { *why = "null inlier array with n > 0"; return ORBX_BAD_ARGUMENT; }
        if (P.model != ORBX_INIT_H && P.model != ORBX_INIT_F) { *why = "model is neither ORBX_INIT_H nor ORBX_INIT_F"; return ORBX_BAD_ARGUMENT; }
        if (!std::isfinite(P.sigma) || !(P.sigma > 0.0f)) { *why = "sigma is not finite or not > 0"; return ORBX_BAD_ARGUMENT; }
        if (const char *w = recon_camera_why(P.K, P.min_parallax)) { *why = w; return ORBX_BAD_ARGUMENT; }
        for (int i = 0; i < P.n; ++i) {
            const int32_t a = P.matches[2 * (size_t)i], b = P.matches[2 * (size_t)i + 1];
            if (a < 0 || a >= P.n1 || b < 0 || b >= P.n2) { *why = "a match index outside its frame"; return ORBX_BAD_ARGUMENT; }
        }
        if (!recon_launches(P)) continue;
        ++plan.nlaunch;
        plan.total_m += (size_t)P.n;
        if (!recon_fits(plan.total_m)) { *why = "too many matches for 32-bit offsets"; return ORBX_UNSUPPORTED; }
    }
    orbx_recon_layout(plan);
    return ORBX_OK;
}

void orbx_recon_pack(const orbx_recon_problem *problems, const OrbxReconPlan &plan, uint8_t *dst) {
    if (plan.nlaunch <= 0) return;
    DReconProb *dp = (DReconProb *)(dst + plan.o_prob);
    float *keys = (float *)(dst + plan.o_keys);
    uint8_t *inl = dst + plan.o_inl;
    int j = 0;
    size_t m_off = 0;
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_recon_problem &P = problems[k];
        if (!recon_launches(P)) continue;
        DReconProb &D = dp[j];
        memset(&D, 0, sizeof(D));
        D.n = P.n; D.is_h = P.model == ORBX_INIT_H ? 1 : 0; D.nhyp = recon_nhyp(P.model);
        D.m_off = (int32_t)m_off; D.key_off = (int32_t)(4 * m_off);
        memcpy(D.M, P.M, sizeof(D.M));
        memcpy(D.K, P.K, sizeof(D.K));
        D.th2 = orbx_recon_th2(P.sigma);
        const size_t n = (size_t)P.n;
        float *pl = keys + 4 * m_off;
        for (size_t i = 0; i < n; ++i) {
            const float *a = P.keys1 + 2 * (size_t)P.matches[2 * i], *b = P.keys2 + 2 * (size_t)P.matches[2 * i + 1];
            pl[i] = a[0]; pl[n + i] = a[1]; pl[2 * n + i] = b[0]; pl[3 * n + i] = b[1];
            inl[m_off + i] = P.inliers[i] ? 1 : 0;
        }
        m_off += n;
        ++j;
    }
}

orbx_status orbx_recon_fused_plan(int nproblems, const orbx_init_problem *problems, const orbx_init_camera *cameras,
                                  OrbxReconPlan &plan, const char **why) {
    plan = OrbxReconPlan();
    plan.nproblems = nproblems; plan.fused = true;
    if (nproblems > 0 && !cameras) { *why = "null camera array"; return ORBX_BAD_ARGUMENT; }
    for (int k = 0; k < nproblems; ++k) {
        if (const char *w = recon_camera_why(cameras[k].K, cameras[k].min_parallax)) { *why = w; return ORBX_BAD_ARGUMENT; }
        if (!orbx_init_launches(problems[k])) continue;
        ++plan.nlaunch;
        plan.total_m += (size_t)problems[k].n;
        if (!recon_fits(plan.total_m)) { *why = "too many matches for 32-bit offsets"; return ORBX_UNSUPPORTED; }
    }
    orbx_recon_layout(plan);
    return ORBX_OK;
}

void orbx_recon_fused_pack(const orbx_init_problem *problems, const orbx_init_camera *cameras, const OrbxReconPlan &plan, uint8_t *dst) {
    DReconProb *dp = (DReconProb *)(dst + plan.o_prob);
    int j = 0;
    size_t m_off = 0;
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_init_problem &P = problems[k];
        if (!orbx_init_launches(P)) continue;
        DReconProb &D = dp[j];
        memset(&D, 0, sizeof(D));                               // is_h, nhyp and M are k_init_select's
        D.n = P.n; D.m_off = (int32_t)m_off;
        D.key_off = (int32_t)((size_t)ORBX_INIT_PLANES * m_off + 4 * (size_t)P.n);   // planes 4 .. 7 of the RANSAC's pts: the raw u1 v1 u2 v2
        memcpy(D.K, cameras[k].K, sizeof(D.K));
        D.th2 = orbx_recon_th2(P.sigma);
        m_off += (size_t)P.n;
        ++j;
    }
}

void orbx_recon_host_run(const OrbxReconPlan &plan, const uint8_t *in, uint8_t *out) {
    const DReconProb *dp = (const DReconProb *)(in + plan.o_prob);
    const float *keys = (const float *)(in + plan.o_keys);
    const uint8_t *inl = in + plan.o_inl;
    OrbxReconPose *pose = (OrbxReconPose *)(out + plan.o_pose);
    OrbxReconTally *tally = (OrbxReconTally *)(out + plan.o_tally);
    int32_t *chosen = (int32_t *)(out + plan.o_chosen);
    uint8_t *st = out + plan.o_st;
    float *pts = (float *)(out + plan.o_pts);
    float ws[ORBX_RECON_WS_FLOATS];
    const OrbxInitWs W = {ws, 1};
    std::vector<uint8_t> hst;
    std::vector<float> hpts;
    std::vector<uint32_t> hkey;
    for (int j = 0; j < plan.nlaunch; ++j) {
        const DReconProb &D = dp[j];
        const size_t n = (size_t)D.n;
        OrbxReconPose *P = pose + (size_t)ORBX_RECON_MAX_HYP * j;
        OrbxReconTally *T = tally + (size_t)ORBX_RECON_MAX_HYP * j;
        memset(P, 0, ORBX_RECON_MAX_HYP * sizeof(OrbxReconPose));
        memset(T, 0, ORBX_RECON_MAX_HYP * sizeof(OrbxReconTally));
        if (D.is_h) orbx_recon_decompose_h(W, D.M, D.K, P);
        else orbx_recon_decompose_f(W, D.M, D.K, P);
        hst.assign(n * D.nhyp, 0);
        hpts.assign(3 * n * D.nhyp, 0.0f);
        const float *pl = keys + D.key_off;
        for (int h = 0; h < D.nhyp; ++h) {
            if (!P[h].valid) continue;
            hkey.clear();
            for (size_t m = 0; m < n; ++m) {
                if (!inl[(size_t)D.m_off + m]) continue;
                float pt[3], c = 0.0f;
                const int s = orbx_recon_check_match(P[h], D.K, D.th2, pl[m], pl[n + m], pl[2 * n + m], pl[3 * n + m], pt, c);
                hst[h * n + m] = (uint8_t)s;
                if (s >= 2) {
                    memcpy(&hpts[3 * (h * n + m)], pt, sizeof(pt));
                    hkey.push_back(orbx_recon_key(c));
                }
            }
            T[h].nGood = (int32_t)hkey.size();
            if (!hkey.empty()) {
                const size_t idx = std::min<size_t>(ORBX_RECON_IDX, hkey.size() - 1);
                std::nth_element(hkey.begin(), hkey.begin() + idx, hkey.end());
                T[h].cosine = orbx_recon_unkey(hkey[idx]);
            }
        }
        const int c = orbx_recon_candidate(D.is_h != 0, T);
        chosen[j] = c;
        if (c >= 0) {
            memcpy(st + D.m_off, &hst[(size_t)c * n], n);
            memcpy(pts + 3 * (size_t)D.m_off, &hpts[3 * (size_t)c * n], 3 * n * sizeof(float));
        } else {
            memset(st + D.m_off, 0, n);
            memset(pts + 3 * (size_t)D.m_off, 0, 3 * n * sizeof(float));
        }
    }
}

static void recon_result_init(OrbxReconResult &S, int32_t n, int32_t model, float min_parallax, int32_t min_triangulated) {
    S.n = n; S.model = model; S.nhyp = recon_nhyp(model);
    S.min_parallax = min_parallax; S.min_triangulated = min_triangulated;
    memset(S.pose, 0, sizeof(S.pose));
    memset(S.tally, 0, sizeof(S.tally));
    memset(S.parallax, 0, sizeof(S.parallax));
    S.status.assign((size_t)n, 0);
    S.points.assign(3 * (size_t)n, 0.0f);
}
orbx_recon_batch *orbx_recon_batch_new(const orbx_recon_problem *problems, const OrbxReconPlan &plan) {
    orbx_recon_batch *b = new orbx_recon_batch();
    b->st.resize((size_t)plan.nproblems);
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_recon_problem &P = problems[k];
        OrbxReconResult &S = b->st[k];
        recon_result_init(S, P.n, P.model, P.min_parallax, P.min_triangulated);
        S.slot = S.launches = recon_launches(P, &S.N);
    }
    return b;
}

// a problem without a model (ORBX_INIT_NONE, or nothing launched) reads as an F problem whose mask is all false
static int32_t recon_winner(const OrbxInitResult &R, const OrbxInitHyp **hyp, const uint64_t **mask) {
    *hyp = nullptr; *mask = nullptr;
    if (!R.launches || R.model == ORBX_INIT_NONE) return ORBX_INIT_F;
    const bool is_h = R.model == ORBX_INIT_H;
    const int off = (is_h || !(R.models & ORBX_INIT_H) ? 0 : R.iterations) + (is_h ? R.itH : R.itF);
    *hyp = &R.hyp[off];
    *mask = R.masks.data() + (size_t)off * R.nwords;
    return R.model;
}

orbx_recon_batch *orbx_recon_batch_new_fused(const orbx_init_camera *cameras, const orbx_init_batch *ib) {
    orbx_recon_batch *b = new orbx_recon_batch();
    b->st.resize(ib->st.size());
    for (size_t k = 0; k < ib->st.size(); ++k) {
        const OrbxInitResult &R = ib->st[k];
        OrbxReconResult &S = b->st[k];
        const OrbxInitHyp *hyp; const uint64_t *mask;
        recon_result_init(S, R.n, recon_winner(R, &hyp, &mask), cameras[k].min_parallax, cameras[k].min_triangulated);
        for (int i = 0; mask && i < R.n; ++i) S.N += (int32_t)((mask[i >> 6] >> (i & 63)) & 1u);
        S.slot = R.launches;
        S.launches = S.N > 0;
    }
    return b;
}

void orbx_recon_problems_from(const orbx_init_problem *problems, const orbx_init_camera *cameras, const orbx_init_batch *ib,
                              std::vector<orbx_recon_problem> &out, std::vector<std::vector<uint8_t>> &store) {
    out.resize(ib->st.size());
    store.resize(ib->st.size());
    for (size_t k = 0; k < ib->st.size(); ++k) {
        const OrbxInitResult &R = ib->st[k];
        const orbx_init_problem &P = problems[k];
        orbx_recon_problem &Q = out[k];
        const OrbxInitHyp *hyp; const uint64_t *mask;
        Q.n1 = P.n1; Q.n2 = P.n2; Q.keys1 = P.keys1; Q.keys2 = P.keys2; Q.n = P.n; Q.matches = P.matches;
        Q.model = recon_winner(R, &hyp, &mask);
        store[k].assign((size_t)P.n + 1, 0);
        if (mask) orbx_unpack_mask(mask, P.n, store[k].data());
        Q.inliers = store[k].data();
        for (int i = 0; i < 9; ++i) Q.M[i] = hyp ? hyp->M[i] : 0.0f;
        memcpy(Q.K, cameras[k].K, sizeof(Q.K));
        Q.sigma = P.sigma; Q.min_parallax = cameras[k].min_parallax; Q.min_triangulated = cameras[k].min_triangulated;
    }
}

// parallax = acos(vCosParallax[idx]) * 180 / CV_PI: the argument is a float and <cmath> is in scope with namespace std, so the
// float overload (acosf) is selected; the product with 180 is a float one, the division by CV_PI a double one, and the result is
// assigned to a float
static float recon_parallax(const OrbxReconTally &T) {
    if (T.nGood <= 0) return 0.0f;
    const float a = acosf(T.cosine) * 180.0f;
    return orbx_canonf((float)((double)a / 3.1415926535897932384626433832795));
}

void orbx_recon_batch_take(orbx_recon_batch *b, const OrbxReconPlan &plan, const uint8_t *out) {
    const OrbxReconPose *pose = (const OrbxReconPose *)(out + plan.o_pose);
    const OrbxReconTally *tally = (const OrbxReconTally *)(out + plan.o_tally);
    const int32_t *chosen = (const int32_t *)(out + plan.o_chosen);
    const uint8_t *st = out + plan.o_st;
    const float *pts = (const float *)(out + plan.o_pts);
    int j = -1;
    size_t m_off = 0, next = 0;
    for (OrbxReconResult &S : b->st) {
        if (!S.slot) continue;
        const size_t n = (size_t)S.n, hyp_off = (size_t)ORBX_RECON_MAX_HYP * ++j;
        m_off = next;
        next += n;
        if (!S.launches) continue;
        memcpy(S.pose, pose + hyp_off, (size_t)S.nhyp * sizeof(OrbxReconPose));
        memcpy(S.tally, tally + hyp_off, (size_t)S.nhyp * sizeof(OrbxReconTally));
        S.chosen = chosen[j];
        S.status.assign(st + m_off, st + m_off + n);
        S.points.assign(pts + 3 * m_off, pts + 3 * (m_off + n));
        for (int i = 0; i < S.nhyp; ++i) S.parallax[i] = S.pose[i].valid ? recon_parallax(S.tally[i]) : 0.0f;
        if (S.model == ORBX_INIT_F) {
            int maxGood = S.tally[0].nGood;
            for (int i = 1; i < 4; ++i) maxGood = std::max(maxGood, S.tally[i].nGood);
            const int nMinGood = std::max(orbx_to_int_clamped(0.9 * S.N), S.min_triangulated);
            int nsimilar = 0;
            for (int i = 0; i < 4; ++i)
                if (S.tally[i].nGood > 0.7 * maxGood) nsimilar++;
            S.ok = 0;
            if (!(maxGood < nMinGood || nsimilar > 1)) S.ok = S.parallax[S.chosen] > S.min_parallax ? 1 : 0;   // chosen: the first i with nGood_i == maxGood
        } else {
            int bestGood = 0, secondBestGood = 0;
            float bestParallax = -1.0f;
            for (int i = 0; i < 8 && S.pose[0].valid; ++i) {
                const int nGood = S.tally[i].nGood;
                if (nGood > bestGood) { secondBestGood = bestGood; bestGood = nGood; bestParallax = S.parallax[i]; }
                else if (nGood > secondBestGood) secondBestGood = nGood;
            }
            S.ok = (secondBestGood < 0.75 * bestGood && bestParallax >= S.min_parallax && bestGood > S.min_triangulated &&
                    bestGood > 0.9 * S.N) ? 1 : 0;
        }
    }
}

orbx_status orbx_recon_get_result(const orbx_recon_batch *b, int k, int32_t *ok, float *R21, float *t21, int32_t *chosen,
                                  uint8_t *status, float *points, int32_t *N, const char **why) {
    const OrbxReconResult *S = orbx_batch_state(b, k, why);
    if (!S) return ORBX_BAD_ARGUMENT;
    if (ok) *ok = S->ok;
    if (R21) { if (S->ok) memcpy(R21, S->pose[S->chosen].R, 9 * sizeof(float)); else memset(R21, 0, 9 * sizeof(float)); }
    if (t21) { if (S->ok) memcpy(t21, S->pose[S->chosen].t, 3 * sizeof(float)); else memset(t21, 0, 3 * sizeof(float)); }
    if (chosen) *chosen = S->chosen;
    if (status && S->n > 0) memcpy(status, S->status.data(), (size_t)S->n);
    if (points && S->n > 0) memcpy(points, S->points.data(), 3 * (size_t)S->n * sizeof(float));
    if (N) *N = S->N;
    return ORBX_OK;
}

orbx_status orbx_recon_get_hypothesis(const orbx_recon_batch *b, int k, int i, float *R9, float *t3, float *n3, int32_t *nGood,
                                      float *cosine, float *parallax, int32_t *valid, const char **why) {
    const OrbxReconResult *S = orbx_batch_state(b, k, why);
    if (!S) return ORBX_BAD_ARGUMENT;
    if (i < 0 || i >= S->nhyp) { *why = "hypothesis outside the problem's model"; return ORBX_BAD_ARGUMENT; }
    if (R9) memcpy(R9, S->pose[i].R, 9 * sizeof(float));
    if (t3) memcpy(t3, S->pose[i].t, 3 * sizeof(float));
    if (n3) memcpy(n3, S->pose[i].n, 3 * sizeof(float));
    if (nGood) *nGood = S->tally[i].nGood;
    if (cosine) *cosine = S->tally[i].cosine;
    if (parallax) *parallax = S->parallax[i];
    if (valid) *valid = S->pose[i].valid;
    return ORBX_OK;
}
