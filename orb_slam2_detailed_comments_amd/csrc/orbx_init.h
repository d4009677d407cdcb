// orbx_init.h -- the H / F RANSAC of Initializer (src/Initializer.cc): Normalize (:1549-1617), ComputeH21 (:497-526), ComputeF21
// (:580-596), the de-normalisation of FindHomography / FindFundamental, CheckHomography (:629-776) and CheckFundamental (:788-942)
// as scalar code shared by the host path (orbx_init.cpp) and the kernels (k_init_hypotheses, k_init_scores).
// tests/init_model.py restates it independently in numpy; DESIGN.md section 2 (F14) lists what was read from the reference's
// source and everything this file fixes for itself where the reference leaves it to OpenCV (cv::SVDecomp, cv::Mat::inv, the
// matrix products).
//
// fp_mode: every expression is written operation by operation and the library is built with -ffp-contract=off, so
// ORBX_FP_GCC_FMA and ORBX_FP_STRICT handles give the same bits, on the host and on the device.  Division and square root are the
// correctly rounded IEEE operations on both sides.  No math library is called.  All arithmetic is float, as the reference's is
// (CV_32F), except the 3 x 3 inverse, which is evaluated in double and rounded once per entry.
// Where the source writes `1.0 / x` and assigns it to a float (sX, sY, invSigmaSquare, w2in1inv, w1in2inv) the division is a
// double one of a float operand and is then rounded to float.  A double carries 53 >= 2 * 24 + 2 bits, so that double rounding
// is innocuous: the value equals the correctly rounded float division 1.0f / x, which is what this file writes.
//
// Every array of the minimal solver lives in ONE workspace of floats that is only reached through OrbxInitWs: element e sits at
// p[e * stride].  The host uses stride 1; k_init_hypotheses gives each lane a lane-interleaved slice of LDS (stride = lanes per
// workgroup), so run-time indices never touch a per-thread array and nothing goes to scratch.
//
// Degenerate and non-finite input runs the same straight-line code, every loop is bounded by a constant, a comparison with a NaN
// is false (so `chi > th` leaves bIn alone and the NaN goes into the score, as in the source); a NaN that is stored is stored as
// the canonical quiet NaN.
#pragma once
#include <vector>
#include "orbx_pose.h"
#include "orbx_ransac.h"

struct OrbxInitHyp {         // one hypothesis as k_init_hypotheses stores it and k_init_scores reads it
    float M[9];              // H21i or F21i, row major
    float Minv[9];           // H12i = H21i.inv(); zeros for F
    int32_t bad, pad;        // 1: an entry of M (for H: or of Minv) is not finite
};
static_assert(sizeof(OrbxInitHyp) == 80, "packed for the device");

enum { ORBX_INIT_SWEEPS = 30,           // sweep cap of the one-sided Jacobi
       ORBX_INIT_HYP_LANES = 64,        // hypotheses (lanes) per workgroup of k_init_hypotheses
       ORBX_INIT_SCORE_LANES = 64,      // hypotheses (lanes) per workgroup of k_init_scores
       ORBX_INIT_CHUNK = 256,           // matches staged in LDS at a time by k_init_scores (4 KiB)
       ORBX_INIT_PLANES = 8 };          // per match: normalised u1 v1 u2 v2 | raw u1 v1 u2 v2
#define ORBX_INIT_SVD_EPS 1e-12f        // a column pair is rotated when gamma^2 > EPS * (alpha * beta): |cos| > 1e-6 ...
#define ORBX_INIT_SVD_TINY 1e-12f       // ... and neither squared norm is below TINY times the other (norm ratio 1e-6)

// workspace layout (floats)
enum { ORBX_INIT_A = 0,                 // 16 x 9 (H) or 8 x 9 (F), row major; afterwards Fpre (3 x 3) at +0 and its V at +9
       ORBX_INIT_V = 144,               // 9 x 9
       ORBX_INIT_PTS = 225,             // the eight drawn matches, normalised: u1 v1 u2 v2 each
       ORBX_INIT_WS_FLOATS = 257 };

struct OrbxInitWs {
    float *p;
    int stride;
    ORBX_HD float &operator()(int e) const { return p[(long long)e * stride]; }
};

ORBX_HD static inline bool orbx_init_finite(float x) {
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    return (b & 0x7f800000u) != 0x7f800000u;
}

// cv::SVDecomp as far as the Initializer needs it, as this library fixes it: one-sided Jacobi in float over the nc columns of
// the m x nc matrix at `a` (row stride nc), V (nc x nc at `v`, row stride nc) accumulated from I.  A sweep visits the column
// pairs (p, q), p < q, row by row: alpha = sum_k a_kp^2, beta = sum_k a_kq^2, gamma = sum_k a_kp a_kq (k ascending, one running
// sum each); the pair is rotated when gamma^2 > ORBX_INIT_SVD_EPS (alpha beta) and alpha > ORBX_INIT_SVD_TINY beta and
// beta > ORBX_INIT_SVD_TINY alpha -- a column that has shrunk to rounding noise beside its partner (the null column of the 8 x 9
// system always does) has a cosine made of noise and would be rotated until the sweep cap --: zeta = (beta - alpha) / (2 gamma),
// t = sgn(zeta) / (|zeta| + sqrt(zeta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c, (a_kp, a_kq) = (c a_kp - s a_kq, s a_kp + c a_kq)
// and the same on V.  The loop ends after a sweep without a rotation and after ORBX_INIT_SWEEPS sweeps.  Returns the column of
// smallest squared norm (sum_k a_kj^2, k ascending; strict <, so the lowest index wins a tie): column j of V is then the right
// singular vector of the smallest singular value -- row nc - 1 of the reference's vt -- and column j of the rotated matrix is
// u_j w_j.  The sign of a vector is left as the rotations give it.
ORBX_HD static inline int orbx_init_jacobi(const OrbxInitWs &W, int a, int v, int m, int nc) {
    for (int i = 0; i < nc; ++i)
        for (int j = 0; j < nc; ++j) W(v + i * nc + j) = i == j ? 1.0f : 0.0f;
    for (int sweep = 0; sweep < ORBX_INIT_SWEEPS; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < nc - 1; ++p)
            for (int q = p + 1; q < nc; ++q) {
                float alpha = 0.0f, beta = 0.0f, gamma = 0.0f;
                for (int k = 0; k < m; ++k) {
                    const float ap = W(a + k * nc + p), aq = W(a + k * nc + q);
                    alpha = alpha + ap * ap;
                    beta = beta + aq * aq;
                    gamma = gamma + ap * aq;
                }
                if (gamma * gamma > ORBX_INIT_SVD_EPS * (alpha * beta) && alpha > ORBX_INIT_SVD_TINY * beta &&
                    beta > ORBX_INIT_SVD_TINY * alpha) {
                    rotated = true;
                    const float zeta = (beta - alpha) / (2.0f * gamma);
                    const float den = __builtin_fabsf(zeta) + sqrtf(zeta * zeta + 1.0f);
                    const float t = (zeta < 0.0f ? -1.0f : 1.0f) / den;
                    const float c = 1.0f / sqrtf(t * t + 1.0f);
                    const float s = t * c;
                    for (int k = 0; k < m; ++k) {
                        const float ap = W(a + k * nc + p), aq = W(a + k * nc + q);
                        W(a + k * nc + p) = c * ap - s * aq;
                        W(a + k * nc + q) = s * ap + c * aq;
                    }
                    for (int k = 0; k < nc; ++k) {
                        const float vp = W(v + k * nc + p), vq = W(v + k * nc + q);
                        W(v + k * nc + p) = c * vp - s * vq;
                        W(v + k * nc + q) = s * vp + c * vq;
                    }
                }
            }
        if (!rotated) break;
    }
    int best = 0;
    float least = 0.0f;
    for (int j = 0; j < nc; ++j) {
        float nj = 0.0f;
        for (int k = 0; k < m; ++k) { const float x = W(a + k * nc + j); nj = nj + x * x; }
        if (j == 0 || nj < least) { least = nj; best = j; }
    }
    return best;
}

// o = a b for row-major 3 x 3 floats, as this library fixes the order: o_ij = (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j
ORBX_HD static inline void orbx_init_mul3(const float *a, const float *b, float *o) {
ORBX_UNROLL
    for (int i = 0; i < 3; ++i) {
ORBX_UNROLL
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
    }
}

// cv::Mat::inv() of a 3 x 3 float matrix, as this library fixes it: the adjugate over the determinant, every product and the
// determinant in double, d = 1 / det, each entry (float)(cofactor * d).  det == 0 is not a special case: d is infinite and every
// entry comes out infinite or NaN.
ORBX_HD static inline void orbx_init_inv3(const float *m, float *o) {
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double k0 = e * i - f * h, k1 = d * i - f * g, k2 = d * h - e * g;
    const double det = (a * k0 - b * k1) + c * k2;
    const double r = 1.0 / det;
    o[0] = (float)(k0 * r);
    o[1] = (float)((c * h - b * i) * r);
    o[2] = (float)((b * f - c * e) * r);
    o[3] = (float)((f * g - d * i) * r);
    o[4] = (float)((a * i - c * g) * r);
    o[5] = (float)((c * d - a * f) * r);
    o[6] = (float)(k2 * r);
    o[7] = (float)((b * g - a * h) * r);
    o[8] = (float)((a * e - b * d) * r);
}

// One iteration of FindHomography (is_h) or FindFundamental up to its check function, for the eight normalised matches at
// ORBX_INIT_PTS: A, its null vector, for F the rank-2 projection, the de-normalisation, for H the inverse.
// T2l is T2inv for H and T2 transposed for F.
ORBX_HD static inline void orbx_init_hypothesis(const OrbxInitWs &W, bool is_h, const float *T1, const float *T2l, OrbxInitHyp &out) {
    const int A = ORBX_INIT_A, V = ORBX_INIT_V, P = ORBX_INIT_PTS;
    for (int i = 0; i < 8; ++i) {
        const float u1 = W(P + 4 * i), v1 = W(P + 4 * i + 1), u2 = W(P + 4 * i + 2), v2 = W(P + 4 * i + 3);
        if (is_h) {
            const int r0 = A + 18 * i, r1 = r0 + 9;
            W(r0) = 0.0f; W(r0 + 1) = 0.0f; W(r0 + 2) = 0.0f;
            W(r0 + 3) = -u1; W(r0 + 4) = -v1; W(r0 + 5) = -1.0f;
            W(r0 + 6) = v2 * u1; W(r0 + 7) = v2 * v1; W(r0 + 8) = v2;
            W(r1) = u1; W(r1 + 1) = v1; W(r1 + 2) = 1.0f;
            W(r1 + 3) = 0.0f; W(r1 + 4) = 0.0f; W(r1 + 5) = 0.0f;
            W(r1 + 6) = -u2 * u1; W(r1 + 7) = -u2 * v1; W(r1 + 8) = -u2;
        } else {
            const int r = A + 9 * i;
            W(r) = u2 * u1; W(r + 1) = u2 * v1; W(r + 2) = u2;
            W(r + 3) = v2 * u1; W(r + 4) = v2 * v1; W(r + 5) = v2;
            W(r + 6) = u1; W(r + 7) = v1; W(r + 8) = 1.0f;
        }
    }
    const int col = orbx_init_jacobi(W, A, V, is_h ? 16 : 8, 9);
    float Mn[9];
    if (is_h) {
ORBX_UNROLL
        for (int i = 0; i < 9; ++i) Mn[i] = W(V + 9 * i + col);                // vt.row(8).reshape(0, 3)
    } else {
        const int G = ORBX_INIT_A, GV = ORBX_INIT_A + 9;                        // A is done with
        for (int i = 0; i < 9; ++i) W(G + i) = W(V + 9 * i + col);              // Fpre
        const int drop = orbx_init_jacobi(W, G, GV, 3, 3);
        // u diag(w) vt with w[2] = 0: column j of the rotated Fpre is u_j w_j, so the product is the sum over the two columns
        // that stay, in ascending order of the column index, of (u_j w_j) v_j^T
        const int c0 = drop == 0 ? 1 : 0, c1 = drop == 2 ? 1 : 2;
ORBX_UNROLL
        for (int i = 0; i < 3; ++i) {
ORBX_UNROLL
            for (int j = 0; j < 3; ++j) Mn[3 * i + j] = W(G + 3 * i + c0) * W(GV + 3 * j + c0) + W(G + 3 * i + c1) * W(GV + 3 * j + c1);
        }
    }
    float tmp[9], M[9];
    orbx_init_mul3(T2l, Mn, tmp);                                               // (T2inv Hn) T1, (T2t Fn) T1
    orbx_init_mul3(tmp, T1, M);
    bool bad = false;
    if (is_h) {
        float Mi[9];
        orbx_init_inv3(M, Mi);
ORBX_UNROLL
        for (int i = 0; i < 9; ++i) { bad = bad || !orbx_init_finite(Mi[i]); out.Minv[i] = orbx_canonf(Mi[i]); }
    } else {
ORBX_UNROLL
        for (int i = 0; i < 9; ++i) out.Minv[i] = 0.0f;
    }
ORBX_UNROLL
    for (int i = 0; i < 9; ++i) { bad = bad || !orbx_init_finite(M[i]); out.M[i] = orbx_canonf(M[i]); }
    out.bad = bad ? 1 : 0;
    out.pad = 0;
}

// invSigmaSquare of both check functions
ORBX_HD static inline float orbx_init_inv_sigma2(float sigma) { return 1.0f / (sigma * sigma); }

// One match of CheckHomography: the two terms are added to `score` in the source's order; returns bIn
ORBX_HD static inline bool orbx_init_check_h(const float *H, const float *Hi, float u1, float v1, float u2, float v2,
                                             float invSigmaSquare, float &score) {
    const float th = (float)5.991;
    bool bIn = true;
    const float w2in1inv = 1.0f / ((Hi[6] * u2 + Hi[7] * v2) + Hi[8]);
    const float u2in1 = ((Hi[0] * u2 + Hi[1] * v2) + Hi[2]) * w2in1inv;
    const float v2in1 = ((Hi[3] * u2 + Hi[4] * v2) + Hi[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false;
    else score = score + (th - chiSquare1);
    const float w1in2inv = 1.0f / ((H[6] * u1 + H[7] * v1) + H[8]);
    const float u1in2 = ((H[0] * u1 + H[1] * v1) + H[2]) * w1in2inv;
    const float v1in2 = ((H[3] * u1 + H[4] * v1) + H[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false;
    else score = score + (th - chiSquare2);
    return bIn;
}

// One match of CheckFundamental
ORBX_HD static inline bool orbx_init_check_f(const float *F, float u1, float v1, float u2, float v2, float invSigmaSquare,
                                             float &score) {
    const float th = (float)3.841, thScore = (float)5.991;
    bool bIn = true;
    const float a2 = (F[0] * u1 + F[1] * v1) + F[2];
    const float b2 = (F[3] * u1 + F[4] * v1) + F[5];
    const float c2 = (F[6] * u1 + F[7] * v1) + F[8];
    const float num2 = (a2 * u2 + b2 * v2) + c2;
    const float squareDist1 = (num2 * num2) / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false;
    else score = score + (thScore - chiSquare1);
    const float a1 = (F[0] * u2 + F[3] * v2) + F[6];
    const float b1 = (F[1] * u2 + F[4] * v2) + F[7];
    const float c1 = (F[2] * u2 + F[5] * v2) + F[8];
    const float num1 = (a1 * u1 + b1 * v1) + c1;
    const float squareDist2 = (num1 * num1) / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false;
    else score = score + (thScore - chiSquare2);
    return bIn;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side (orbx_init.cpp, HIP-free): validation, Normalize, packing, the host path, the result object.
struct DInitProb {                  // one problem that launches, as the kernels read it
    int32_t n, iterations, nwords, models;   // nwords = ceil(n / 64); models = ORBX_INIT_H | ORBX_INIT_F
    int32_t hyp_off;                // first hypothesis / score: [H: iterations][F: iterations], a model not requested is absent
    int32_t pts_off;                // first float of its ORBX_INIT_PLANES planes of n floats
    int32_t word_off;               // first mask word: [hypotheses][nwords]
    int32_t set_off;                // first set index: [iterations][8]
    float T1[9], T2inv[9], T2t[9];
    float inv_sigma2;
};
static_assert(sizeof(DInitProb) == 144, "packed for the device");
ORBX_HD static inline int orbx_init_nhyp(const DInitProb &D) { return D.iterations * ((D.models & 1) + ((D.models >> 1) & 1)); }
// hypothesis l of a problem: which model, which iteration
ORBX_HD static inline bool orbx_init_is_h(const DInitProb &D, int l) { return (D.models & 1) && l < D.iterations; }
ORBX_HD static inline int orbx_init_iteration(const DInitProb &D, int l) { return l < D.iterations ? l : l - D.iterations; }
// sets: [iterations][8] per problem, shared by its H and F hypotheses; a group: ORBX_INIT_SCORE_LANES hypotheses of
// k_init_scores; tally: the scores
using DInitArgs = DRansacArgs<DInitProb, OrbxInitHyp, float>;
using OrbxInitPlan = OrbxRansacPlan;
// a problem that has hypotheses to compute; any other launches nothing and reports ORBX_INIT_NONE
static inline bool orbx_init_launches(const orbx_init_problem &P) { return P.n >= 8 && P.models != 0; }
orbx_status orbx_init_plan(int nproblems, const orbx_init_problem *problems, OrbxInitPlan &plan, const char **why);
void orbx_init_pack(const orbx_init_problem *problems, const OrbxInitPlan &plan, uint8_t *dst);
// the host path: reads the packed block, writes the downloaded block's layout (hyp | masks | scores) into out
void orbx_init_host_run(const OrbxInitPlan &plan, const uint8_t *in, uint8_t *out);

struct OrbxInitResult {             // one problem of a batch
    int32_t n = 0, iterations = 0, nwords = 0, models = 0;
    bool launches = false;          // false: n < 8, nothing is computed
    float T1[9], T2[9];
    std::vector<OrbxInitHyp> hyp;   // [H: iterations][F: iterations] as far as requested
    std::vector<float> scores;
    std::vector<uint64_t> masks;
    float SH = 0.0f, SF = 0.0f, RH = 0.0f;
    int32_t itH = -1, itF = -1, model = 0;
};
struct orbx_init_batch {
    std::vector<OrbxInitResult> st;
};
// results with Normalize done and nothing stored; orbx_init_batch_take scatters a downloaded block into them and picks the bests
orbx_init_batch *orbx_init_batch_new(const orbx_init_problem *problems, const OrbxInitPlan &plan);
void orbx_init_batch_take(orbx_init_batch *b, const OrbxInitPlan &plan, const uint8_t *out);
orbx_status orbx_init_get_result(const orbx_init_batch *b, int k, float *SH, float *SF, float *H21, float *F21, uint8_t *inliersH,
                                 uint8_t *inliersF, int32_t *itH, int32_t *itF, float *RH, int32_t *model, const char **why);
orbx_status orbx_init_get_scores(const orbx_init_batch *b, int k, int model, float *scores, int32_t *niterations, const char **why);
orbx_status orbx_init_get_hypothesis(const orbx_init_batch *b, int k, int model, int iteration, float *M9, float *Minv9, float *score,
                                     uint64_t *mask_words, const char **why);
orbx_status orbx_init_get_normalization(const orbx_init_batch *b, int k, float *T1, float *T2, const char **why);
