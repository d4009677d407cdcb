// orbx_recon.h -- what turns the winning H or F of the Initializer (src/Initializer.cc) into a map: ReconstructF (:963-1132),
// ReconstructH (:1154-1462), DecomposeE (:1838-1869), CheckRT (:1636-1824) and Triangulate (:1473-1526) as scalar code shared by
// the host path (orbx_recon.cpp) and the kernels (k_init_decompose, k_init_check_rt, k_init_pick; k_init_select joins them to the
// RANSAC's kernels in the fused call).  tests/recon_model.py restates
// it independently in numpy; DESIGN.md section 2 (F15) lists what was read from the reference's source and everything this file
// fixes for itself where the reference leaves it to OpenCV or libm (cv::SVD::compute, cv::determinant, cv::norm, Mat::dot, the
// matrix products, Mat / scalar, std::sort, acos).
//
// fp_mode: every expression is written operation by operation and the library is built with -ffp-contract=off, so
// ORBX_FP_GCC_FMA and ORBX_FP_STRICT handles give the same bits, on the host and on the device.  Division and square root are the
// correctly rounded IEEE operations on both sides.  No math library is called on the device: acos runs on the host, once per pose
// hypothesis, on the cosine the device selected.
//
// LDS: k_init_decompose gives each lane ORBX_RECON_WS_FLOATS floats of a lane-interleaved workspace (the 3 x 3 SVD picks its
// columns at run time): ORBX_RECON_WS_FLOATS * ORBX_RECON_LANES * 4 = 4608 bytes per workgroup.  k_init_check_rt, k_init_pick and
// k_init_select use none: the 4 x 4 Jacobi of Triangulate runs in registers.  No kernel uses scratch.
//
// Degenerate and non-finite input (dist1 * dist2 == 0, non-finite keypoints, a singular K) runs the same straight-line code, every
// loop is bounded by a constant, a comparison with a NaN is false wherever the source compares, and a NaN that is stored is stored
// as the canonical quiet NaN.
#pragma once
#include <vector>
#include "orbx_init.h"

enum { ORBX_RECON_LANES = 64,           // problems (lanes) per workgroup of k_init_decompose
       ORBX_RECON_WS_FLOATS = 18,       // the 3 x 3 matrix and its V
       ORBX_RECON_MAX_HYP = 8,          // pose hypotheses of ReconstructH; ReconstructF has 4
       ORBX_RECON_IDX = 50 };           // idx = min(50, size - 1) of the ascending cosines

struct OrbxReconPose {                  // one pose hypothesis as k_init_decompose stores it and k_init_check_rt reads it
    float R[9], t[3], n[3];             // n: the plane normal of ReconstructH, zeros for F
    float P2[12], O2[3];                // K [R | t], -R^T t
    int32_t valid, pad;                 // valid 0: the d1 / d2, d2 / d3 test of ReconstructH returned false before any hypothesis
};
static_assert(sizeof(OrbxReconPose) == 128, "packed for the device");
struct OrbxReconTally { int32_t nGood; float cosine; };   // cosine: vCosParallax[idx] after the sort; 0 when nGood == 0
static_assert(sizeof(OrbxReconTally) == 8, "packed for the device");

// cv::determinant of a 3 x 3 float matrix, as this library fixes it: every product and sum in double, (a k0 - b k1) + c k2
ORBX_HD static inline double orbx_recon_det3(const float *m) {
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double k0 = e * i - f * h, k1 = d * i - f * g, k2 = d * h - e * g;
    return (a * k0 - b * k1) + c * k2;
}
// cv::norm of a 3-vector (the rule of F12): the squares summed in double in index order, IEEE square root
ORBX_HD static inline double orbx_recon_norm3(float x, float y, float z) {
    const double a = x, b = y, c = z;
    return sqrt((a * a + b * b) + c * c);
}
// Mat / scalar: each entry divided by the scalar in double and rounded to float once
ORBX_HD static inline float orbx_recon_div(float x, double s) { return (float)((double)x / s); }
// a 3 x 3 matrix times a 3-vector: (m_i0 x + m_i1 y) + m_i2 z in float
ORBX_HD static inline void orbx_recon_mulv(const float *m, float x, float y, float z, float *o) {
ORBX_UNROLL
    for (int i = 0; i < 3; ++i) o[i] = (m[3 * i] * x + m[3 * i + 1] * y) + m[3 * i + 2] * z;
}

// cv::SVD::compute of a 3 x 3 float matrix with U, w and Vt, as this library fixes it.  orbx_init_jacobi over the three columns
// of M: afterwards column j of the rotated matrix is u_j w_j and column j of V is v_j.  The squared norms n_j (sum over the rows
// in ascending order) are sorted descending by three compare-and-swap steps on neighbours, (0,1) (1,2) (0,1), each swapping when
// the later one is strictly larger: a tie keeps the lower column first, a NaN stays where it is.  w = sqrt(n).  u_0 and u_1 are
// their rotated columns divided by w_0 and w_1 in float.  u_2 is NOT its column over w_2 -- for the rank-2 E that would be noise
// over noise --: u_2 = u_0 x u_1, each entry a b - c d in float, negated when its dot product (float, index order) with the third
// rotated column is < 0, so that U diag(w) Vt is M for a matrix of full rank too.  Vt row i is the column of V that goes with w_i.
// The signs of u_0, u_1 and of V are left as the rotations give them.
struct OrbxReconSvd { float U[9], w[3], Vt[9]; };
ORBX_HD static inline void orbx_recon_svd3(const OrbxInitWs &W, const float *M, OrbxReconSvd &S) {
    const int A = 0, V = 9;
ORBX_UNROLL
    for (int i = 0; i < 9; ++i) W(A + i) = M[i];
    orbx_init_jacobi(W, A, V, 3, 3);
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
ORBX_UNROLL
    for (int k = 0; k < 3; ++k) {
        const float a = W(A + 3 * k), b = W(A + 3 * k + 1), c = W(A + 3 * k + 2);
        n0 = n0 + a * a;
        n1 = n1 + b * b;
        n2 = n2 + c * c;
    }
    int i0 = 0, i1 = 1, i2 = 2;
    if (n1 > n0) { const float f = n0; n0 = n1; n1 = f; const int i = i0; i0 = i1; i1 = i; }
    if (n2 > n1) { const float f = n1; n1 = n2; n2 = f; const int i = i1; i1 = i2; i2 = i; }
    if (n1 > n0) { const float f = n0; n0 = n1; n1 = f; const int i = i0; i0 = i1; i1 = i; }
    S.w[0] = sqrtf(n0); S.w[1] = sqrtf(n1); S.w[2] = sqrtf(n2);
    float c2[3];
ORBX_UNROLL
    for (int k = 0; k < 3; ++k) {
        S.U[3 * k] = W(A + 3 * k + i0) / S.w[0];
        S.U[3 * k + 1] = W(A + 3 * k + i1) / S.w[1];
        c2[k] = W(A + 3 * k + i2);
        S.Vt[k] = W(V + 3 * k + i0);
        S.Vt[3 + k] = W(V + 3 * k + i1);
        S.Vt[6 + k] = W(V + 3 * k + i2);
    }
    float x = S.U[3] * S.U[7] - S.U[6] * S.U[4];               // u_0 x u_1
    float y = S.U[6] * S.U[1] - S.U[0] * S.U[7];
    float z = S.U[0] * S.U[4] - S.U[3] * S.U[1];
    const float d = (x * c2[0] + y * c2[1]) + z * c2[2];
    if (d < 0.0f) { x = -x; y = -y; z = -z; }
    S.U[2] = x; S.U[5] = y; S.U[8] = z;
}

// P2 = K [R | t] and O2 = -R^T t of CheckRT for a pose whose R and t are set.  K9 is the 3 x 3 K with its zeros and its one; each
// entry of P2 is (K_i0 X_0j + K_i1 X_1j) + K_i2 X_2j, each entry of O2 ((-R_0i) t_0 + (-R_1i) t_1) + (-R_2i) t_2.
ORBX_HD static inline void orbx_recon_pose_finish(const float *K9, OrbxReconPose &P) {
ORBX_UNROLL
    for (int i = 0; i < 3; ++i) {
ORBX_UNROLL
        for (int j = 0; j < 4; ++j) {
            const float x0 = j < 3 ? P.R[j] : P.t[0], x1 = j < 3 ? P.R[3 + j] : P.t[1], x2 = j < 3 ? P.R[6 + j] : P.t[2];
            P.P2[4 * i + j] = orbx_canonf((K9[3 * i] * x0 + K9[3 * i + 1] * x1) + K9[3 * i + 2] * x2);
        }
        P.O2[i] = orbx_canonf(((-P.R[i]) * P.t[0] + (-P.R[3 + i]) * P.t[1]) + (-P.R[6 + i]) * P.t[2]);
    }
ORBX_UNROLL
    for (int i = 0; i < 9; ++i) P.R[i] = orbx_canonf(P.R[i]);
ORBX_UNROLL
    for (int i = 0; i < 3; ++i) { P.t[i] = orbx_canonf(P.t[i]); P.n[i] = orbx_canonf(P.n[i]); }
}
ORBX_HD static inline void orbx_recon_K9(const float *K4, float *K9) {
    K9[0] = K4[0]; K9[1] = 0.0f; K9[2] = K4[2];
    K9[3] = 0.0f; K9[4] = K4[1]; K9[5] = K4[3];
    K9[6] = 0.0f; K9[7] = 0.0f; K9[8] = 1.0f;
}

// ReconstructF up to its CheckRT calls: E21 = (K^T F21) K, DecomposeE, the four poses in the order (R1, t) (R2, t) (R1, -t)
// (R2, -t).  DecomposeE: t = u.col(2) / cv::norm(u.col(2)); R1 = (u W) vt, negated when its determinant is < 0;
// R2 = (u W^T) vt likewise.
ORBX_HD static inline void orbx_recon_decompose_f(const OrbxInitWs &W, const float *F21, const float *K4, OrbxReconPose *out) {
    float K9[9], Kt[9], tmp[9], E[9];
    orbx_recon_K9(K4, K9);
ORBX_UNROLL
    for (int i = 0; i < 3; ++i) {
ORBX_UNROLL
        for (int j = 0; j < 3; ++j) Kt[3 * i + j] = K9[3 * j + i];
    }
    orbx_init_mul3(Kt, F21, tmp);
    orbx_init_mul3(tmp, K9, E);
    OrbxReconSvd S;
    orbx_recon_svd3(W, E, S);
    const double nt = orbx_recon_norm3(S.U[2], S.U[5], S.U[8]);
    const float t[3] = {orbx_recon_div(S.U[2], nt), orbx_recon_div(S.U[5], nt), orbx_recon_div(S.U[8], nt)};
    const float Wm[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    const float Wt[9] = {0.0f, 1.0f, 0.0f, -1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float R1[9], R2[9];
    orbx_init_mul3(S.U, Wm, tmp);
    orbx_init_mul3(tmp, S.Vt, R1);
    if (orbx_recon_det3(R1) < 0.0) {
ORBX_UNROLL
        for (int i = 0; i < 9; ++i) R1[i] = -R1[i];
    }
    orbx_init_mul3(S.U, Wt, tmp);
    orbx_init_mul3(tmp, S.Vt, R2);
    if (orbx_recon_det3(R2) < 0.0) {
ORBX_UNROLL
        for (int i = 0; i < 9; ++i) R2[i] = -R2[i];
    }
ORBX_UNROLL
    for (int h = 0; h < 4; ++h) {
        OrbxReconPose P;
ORBX_UNROLL
        for (int i = 0; i < 9; ++i) P.R[i] = (h & 1) ? R2[i] : R1[i];
ORBX_UNROLL
        for (int i = 0; i < 3; ++i) { P.t[i] = h < 2 ? t[i] : -t[i]; P.n[i] = 0.0f; }
        P.valid = 1; P.pad = 0;
        orbx_recon_pose_finish(K9, P);
        out[h] = P;
    }
}

// ReconstructH up to its CheckRT calls: A = (Kinv H21) K, its SVD, s = (float)(det(U) det(Vt)), the early return, and the eight
// (R, t, n) in the source's order: R = s ((U Rp) Vt), t = U tp divided by its cv::norm, n = V np, negated when n[2] < 0.
// Returns false, with all eight records zero and invalid, when d1 / d2 < 1.00001 || d2 / d3 < 1.00001 (a float quotient against
// the double literal).
ORBX_HD static inline bool orbx_recon_decompose_h(const OrbxInitWs &W, const float *H21, const float *K4, OrbxReconPose *out) {
    float K9[9], Ki[9], tmp[9], A[9];
    orbx_recon_K9(K4, K9);
    orbx_init_inv3(K9, Ki);
    orbx_init_mul3(Ki, H21, tmp);
    orbx_init_mul3(tmp, K9, A);
    OrbxReconSvd S;
    orbx_recon_svd3(W, A, S);
    const float s = (float)(orbx_recon_det3(S.U) * orbx_recon_det3(S.Vt));
    const float d1 = S.w[0], d2 = S.w[1], d3 = S.w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) {
ORBX_UNROLL
        for (int h = 0; h < 8; ++h) {
            OrbxReconPose P;
ORBX_UNROLL
            for (int i = 0; i < 9; ++i) P.R[i] = 0.0f;
ORBX_UNROLL
            for (int i = 0; i < 3; ++i) { P.t[i] = 0.0f; P.n[i] = 0.0f; P.O2[i] = 0.0f; }
ORBX_UNROLL
            for (int i = 0; i < 12; ++i) P.P2[i] = 0.0f;
            P.valid = 0; P.pad = 0;
            out[h] = P;
        }
        return false;
    }
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
ORBX_UNROLL
    for (int h = 0; h < 8; ++h) {
        const int i = h & 3;
        const bool second = h >= 4;
        const float x1 = i < 2 ? aux1 : -aux1, x3 = (i & 1) ? -aux3 : aux3;
        const float aux_s = second ? aux_sphi : aux_stheta;
        const float sn = (i == 0 || i == 3) ? aux_s : -aux_s;           // stheta[i], sphi[i]
        float Rp[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
        float tp[3];
        if (!second) {
            Rp[0] = ctheta; Rp[2] = -sn; Rp[6] = sn; Rp[8] = ctheta;
            tp[0] = x1 * (d1 - d3); tp[1] = 0.0f * (d1 - d3); tp[2] = (-x3) * (d1 - d3);
        } else {
            Rp[0] = cphi; Rp[2] = sn; Rp[4] = -1.0f; Rp[6] = sn; Rp[8] = -cphi;
            tp[0] = x1 * (d1 + d3); tp[1] = 0.0f * (d1 + d3); tp[2] = x3 * (d1 + d3);
        }
        OrbxReconPose P;
        float UR[9], R[9], t[3];
        orbx_init_mul3(S.U, Rp, UR);
        orbx_init_mul3(UR, S.Vt, R);
ORBX_UNROLL
        for (int k = 0; k < 9; ++k) P.R[k] = s * R[k];
        orbx_recon_mulv(S.U, tp[0], tp[1], tp[2], t);
        const double nt = orbx_recon_norm3(t[0], t[1], t[2]);
ORBX_UNROLL
        for (int k = 0; k < 3; ++k) P.t[k] = orbx_recon_div(t[k], nt);
        float n[3];
ORBX_UNROLL
        for (int k = 0; k < 3; ++k) n[k] = (S.Vt[k] * x1 + S.Vt[3 + k] * 0.0f) + S.Vt[6 + k] * x3;   // V np, V = Vt^T
        const bool flip = n[2] < 0.0f;
ORBX_UNROLL
        for (int k = 0; k < 3; ++k) P.n[k] = flip ? -n[k] : n[k];
        P.valid = 1; P.pad = 0;
        orbx_recon_pose_finish(K9, P);
        out[h] = P;
    }
    return true;
}

// th2 of the CheckRT calls: 4.0 * mSigma2 formed in double, passed as float; mSigma2 = sigma * sigma in float
ORBX_HD static inline float orbx_recon_th2(float sigma) { return (float)(4.0 * (double)(sigma * sigma)); }

// One inlier match of CheckRT, with Triangulate: returns the status byte -- 0: rejected by a depth or reprojection test (nothing
// happens), 1: the point is not finite (vbGood[first] = false), 2: counted (nGood, the point, the cosine), 3: counted and
// vbGood[first] = true -- and for 2 and 3 the point and the cosine.
// Triangulate: the four rows of A in float from P1 = [K | 0] and P2, the null vector by orbx_init_jacobi with m = nc = 4 on a
// workspace of this function's own (every index is a constant once the loops are unrolled, so it lives in registers), the column of V
// chosen by selects, x3D = its first three entries, each divided by the fourth in float.
ORBX_HD static inline int orbx_recon_check_match(const OrbxReconPose &P, const float *K4, float th2, float u1, float v1, float u2,
                                                 float v2, float *pt, float &cosine) {
    float K9[9];
    orbx_recon_K9(K4, K9);
    float ws[32];
    const OrbxInitWs W = {ws, 1};
ORBX_UNROLL
    for (int j = 0; j < 4; ++j) {
        const float p10 = j < 3 ? K9[j] : 0.0f, p11 = j < 3 ? K9[3 + j] : 0.0f, p12 = j < 3 ? K9[6 + j] : 0.0f;
        ws[j] = u1 * p12 - p10;
        ws[4 + j] = v1 * p12 - p11;
        ws[8 + j] = u2 * P.P2[8 + j] - P.P2[j];
        ws[12 + j] = v2 * P.P2[8 + j] - P.P2[4 + j];
    }
    const int col = orbx_init_jacobi(W, 0, 16, 4, 4);
    float x[4];
ORBX_UNROLL
    for (int i = 0; i < 4; ++i)
        x[i] = col == 0 ? ws[16 + 4 * i] : col == 1 ? ws[17 + 4 * i] : col == 2 ? ws[18 + 4 * i] : ws[19 + 4 * i];
    const float X = x[0] / x[3], Y = x[1] / x[3], Z = x[2] / x[3];
    if (!orbx_init_finite(X) || !orbx_init_finite(Y) || !orbx_init_finite(Z)) return 1;
    const float a0 = X - 0.0f, a1 = Y - 0.0f, a2 = Z - 0.0f;            // normal1 = p3dC1 - O1
    const float dist1 = (float)orbx_recon_norm3(a0, a1, a2);
    const float b0 = X - P.O2[0], b1 = Y - P.O2[1], b2 = Z - P.O2[2];
    const float dist2 = (float)orbx_recon_norm3(b0, b1, b2);
    const double dot = ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;   // Mat::dot
    const float cosParallax = (float)(dot / (double)(dist1 * dist2));
    const bool low = (double)cosParallax < 0.99998;
    if (Z <= 0.0f && low) return 0;
    float p2[3];
    orbx_recon_mulv(P.R, X, Y, Z, p2);
    p2[0] = p2[0] + P.t[0]; p2[1] = p2[1] + P.t[1]; p2[2] = p2[2] + P.t[2];
    if (p2[2] <= 0.0f && low) return 0;
    const float fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    const float invZ1 = 1.0f / Z;
    const float im1x = fx * X * invZ1 + cx, im1y = fy * Y * invZ1 + cy;
    const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    if (squareError1 > th2) return 0;
    const float invZ2 = 1.0f / p2[2];
    const float im2x = fx * p2[0] * invZ2 + cx, im2y = fy * p2[1] * invZ2 + cy;
    const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    if (squareError2 > th2) return 0;
    pt[0] = X; pt[1] = Y; pt[2] = Z;
    cosine = orbx_canonf(cosParallax);
    return low ? 3 : 2;
}

// The order statistic of CheckRT is defined by value, on the monotone integer key of the float: negative floats in descending
// order of their bits, then the positive ones ascending.  -0 sorts before +0 and the canonical NaN (the only NaN that is stored)
// after +infinity: a total order where std::sort has none.
ORBX_HD static inline uint32_t orbx_recon_key(float x) {
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
ORBX_HD static inline float orbx_recon_unkey(uint32_t k) {
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float x;
    __builtin_memcpy(&x, &b, 4);
    return x;
}
// which hypothesis can win, from the counts alone: ReconstructF -- the first i with nGood_i == maxGood; ReconstructH -- the first
// strict maximum from bestGood = 0, -1 when every count is 0
ORBX_HD static inline int orbx_recon_candidate(bool is_h, const OrbxReconTally *T) {
    int best = is_h ? -1 : 0, most = is_h ? 0 : T[0].nGood;
    const int nh = is_h ? 8 : 4;
    for (int i = is_h ? 0 : 1; i < nh; ++i)
        if (T[i].nGood > most) { most = T[i].nGood; best = i; }
    return best;
}

// Initialize's choice between the models (:204 to its return) from the two best scores and their iterations, as
// orbx_init_batch_take makes it: RH = SH / (SH + SF) in float, ORBX_INIT_NONE when neither model has an iteration above 0, else H
// iff (double)RH > 0.40
ORBX_HD static inline int orbx_recon_choose(float SH, float SF, int itH, int itF) {
    const float RH = SH / (SH + SF);
    if (itH < 0 && itF < 0) return ORBX_INIT_NONE;
    return (double)RH > 0.40 ? ORBX_INIT_H : ORBX_INIT_F;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side (orbx_recon.cpp, HIP-free): validation, packing, the host path, acos and the accept / reject arithmetic, the result.
// Every problem that launches has ORBX_RECON_MAX_HYP slots (pose records, tallies, per-hypothesis planes), whatever its model:
// slot 8 j + i belongs to hypothesis i of launching problem j, and a wave whose i is not below the problem's nhyp returns at once.
// The fused call (orbx_initialize_batch_create) learns the model on the device, so the slots cannot depend on it.
struct DReconProb {                 // one problem that launches, as the kernels read it
    int32_t n, is_h, nhyp;          // nhyp = 8 (H), 4 (F); fused call, set by k_init_select: also 0 (ORBX_INIT_NONE)
    int32_t m_off;                  // first match: the inlier and the downloaded status bytes start at byte m_off, the downloaded
                                    // points at float 3 * m_off, the per-hypothesis planes at match 8 * m_off
    int32_t key_off;                // first float of its u1 | v1 | u2 | v2 planes of n floats
    float M[9], K[4], th2;
    int32_t pad;
};
static_assert(sizeof(DReconProb) == 80, "packed for the device");
struct OrbxReconPlan {
    int nproblems = 0, nlaunch = 0;
    bool fused = false;             // fused call: only the records are uploaded, the keys are the RANSAC's planes, the inlier bytes
                                    // are written by k_init_select into the work block
    size_t total_m = 0;
    size_t o_prob = 0, o_keys = 0, o_inl = 0, in_bytes = 0;                             // uploaded
    size_t o_all_st = 0, o_all_pts = 0, o_all_cos = 0, o_winl = 0, work_bytes = 0;      // device only
    size_t o_pose = 0, o_tally = 0, o_chosen = 0, o_st = 0, o_pts = 0, out_bytes = 0;   // downloaded
};
static inline void orbx_recon_layout(OrbxReconPlan &p) {
    const size_t slots = (size_t)p.nlaunch * ORBX_RECON_MAX_HYP, all = p.total_m * ORBX_RECON_MAX_HYP;
    p.o_prob = 0;
    p.o_keys = orbx_pad256((size_t)p.nlaunch * sizeof(DReconProb));
    p.o_inl = p.o_keys + (p.fused ? 0 : orbx_pad256(p.total_m * 4 * sizeof(float)));
    p.in_bytes = p.o_inl + (p.fused ? 0 : orbx_pad256(p.total_m));
    p.o_all_st = 0;
    p.o_all_pts = orbx_pad256(all);
    p.o_all_cos = p.o_all_pts + orbx_pad256(all * 3 * sizeof(float));
    p.o_winl = p.o_all_cos + orbx_pad256(all * sizeof(float));
    p.work_bytes = p.o_winl + (p.fused ? orbx_pad256(p.total_m) : 0);
    p.o_pose = 0;
    p.o_tally = orbx_pad256(slots * sizeof(OrbxReconPose));
    p.o_chosen = p.o_tally + orbx_pad256(slots * sizeof(OrbxReconTally));
    p.o_st = p.o_chosen + orbx_pad256((size_t)p.nlaunch * sizeof(int32_t));
    p.o_pts = p.o_st + orbx_pad256(p.total_m);
    p.out_bytes = p.o_pts + orbx_pad256(p.total_m * 3 * sizeof(float));
}
struct DReconArgs {                 // what the kernels get, by value
    DReconProb *prob;               // (written by k_init_select only)
    const float *keys;
    uint8_t *inl;                   // (written by k_init_select only)
    uint8_t *all_st; float *all_pts, *all_cos;
    OrbxReconPose *pose; OrbxReconTally *tally; int32_t *chosen; uint8_t *st; float *pts;
    int nlaunch;
};
// init_pts: the fused call's key planes (the pts of the RANSAC's uploaded block); null for the stand-alone call
static inline DReconArgs orbx_recon_args(const OrbxReconPlan &p, uint8_t *in, uint8_t *work, uint8_t *out, const float *init_pts) {
    DReconArgs a;
    a.prob = (DReconProb *)(in + p.o_prob);
    a.keys = p.fused ? init_pts : (const float *)(in + p.o_keys);
    a.inl = p.fused ? work + p.o_winl : in + p.o_inl;
    a.all_st = work + p.o_all_st; a.all_pts = (float *)(work + p.o_all_pts); a.all_cos = (float *)(work + p.o_all_cos);
    a.pose = (OrbxReconPose *)(out + p.o_pose); a.tally = (OrbxReconTally *)(out + p.o_tally);
    a.chosen = (int32_t *)(out + p.o_chosen); a.st = out + p.o_st; a.pts = (float *)(out + p.o_pts);
    a.nlaunch = p.nlaunch;
    return a;
}
orbx_status orbx_recon_plan(int nproblems, const orbx_recon_problem *problems, OrbxReconPlan &plan, const char **why);
void orbx_recon_pack(const orbx_recon_problem *problems, const OrbxReconPlan &plan, uint8_t *dst);
// the host path: reads the packed block, writes the downloaded block's layout into out
void orbx_recon_host_run(const OrbxReconPlan &plan, const uint8_t *in, uint8_t *out);
// the fused call: the cameras are validated, every problem of the RANSAC that launches gets a record (n, offsets, K, th2; the
// model, the matrix and the inlier bytes are k_init_select's)
orbx_status orbx_recon_fused_plan(int nproblems, const orbx_init_problem *problems, const orbx_init_camera *cameras,
                                  OrbxReconPlan &plan, const char **why);
void orbx_recon_fused_pack(const orbx_init_problem *problems, const orbx_init_camera *cameras, const OrbxReconPlan &plan, uint8_t *dst);

struct OrbxReconResult {            // one problem of a batch
    int32_t n = 0, N = 0, model = 0, nhyp = 0, chosen = -1, ok = 0;
    bool slot = false;              // has slots in the downloaded block
    bool launches = false;          // ... and they hold a reconstruction (fused call: not ORBX_INIT_NONE, not an all-false mask)
    float min_parallax = 0.0f; int32_t min_triangulated = 0;
    OrbxReconPose pose[ORBX_RECON_MAX_HYP];
    OrbxReconTally tally[ORBX_RECON_MAX_HYP];
    float parallax[ORBX_RECON_MAX_HYP];
    std::vector<uint8_t> status;
    std::vector<float> points;
};
struct orbx_recon_batch {
    std::vector<OrbxReconResult> st;
};
orbx_recon_batch *orbx_recon_batch_new(const orbx_recon_problem *problems, const OrbxReconPlan &plan);
// the fused call, after orbx_init_batch_take: model and N come from the RANSAC's results
orbx_recon_batch *orbx_recon_batch_new_fused(const orbx_init_camera *cameras, const orbx_init_batch *ib);
// the stand-alone problems that continue a RANSAC batch: its winning matrix and mask per problem (`store` owns the copies);
// a problem whose model is ORBX_INIT_NONE gets n = 0 and reconstructs nothing
void orbx_recon_problems_from(const orbx_init_problem *problems, const orbx_init_camera *cameras, const orbx_init_batch *ib,
                              std::vector<orbx_recon_problem> &out, std::vector<std::vector<uint8_t>> &store);
// scatters a downloaded block into the results, runs acos and the accept / reject arithmetic of ReconstructH / ReconstructF
void orbx_recon_batch_take(orbx_recon_batch *b, const OrbxReconPlan &plan, const uint8_t *out);
orbx_status orbx_recon_get_result(const orbx_recon_batch *b, int k, int32_t *ok, float *R21, float *t21, int32_t *chosen,
                                  uint8_t *status, float *points, int32_t *N, const char **why);
orbx_status orbx_recon_get_hypothesis(const orbx_recon_batch *b, int k, int i, float *R9, float *t3, float *n3, int32_t *nGood,
                                      float *cosine, float *parallax, int32_t *valid, const char **why);
