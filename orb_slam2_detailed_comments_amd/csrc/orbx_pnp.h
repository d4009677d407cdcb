// orbx_pnp.h -- PnPsolver (src/PnPsolver.cc): compute_pose, i.e. EPnP (:543-1510), and CheckInliers (:444-481) as scalar code
// shared by the host path (orbx_pnp.cpp) and the kernels (k_pnp_hypotheses, k_pnp_inliers).  tests/pnp_model.py restates it
// independently in numpy; DESIGN.md section 2 (F13) lists what was read from the reference's source and everything this file
// fixes for itself where the reference leaves it to OpenCV 1.x C calls (cvSVD, cvInvert, cvSolve, cvMulTransposed).
//
// fp_mode: every expression is written operation by operation and the library is built with -ffp-contract=off, so
// ORBX_FP_GCC_FMA and ORBX_FP_STRICT handles give the same bits, on the host and on the device.  Division and square root are
// the correctly rounded IEEE operations on both sides.  No math library is called.
//
// Every array of the algorithm lives in ONE workspace of doubles that is only reached through OrbxPnpWs: element e sits at
// p[e * stride].  The host uses stride 1; k_pnp_hypotheses gives each lane a lane-interleaved slice of LDS (stride = lanes per
// workgroup), so run-time indices never touch a per-thread array and nothing goes to scratch.
//
// OUTSIDE the contract (a negative eigenvalue under sqrt, the singular branch of qr_solve, betas[0] == 0, z == 0, non-finite
// input): the same code runs, every loop is bounded by a constant, qr_solve's singular branch gives X = 0, a non-finite error2
// compares as "not less" and the point is an outlier; a NaN that is stored is stored as the canonical quiet NaN.
#pragma once
#include <vector>
#include "orbx_pose.h"
#include "orbx_ransac.h"

struct OrbxPnpHyp {          // one hypothesis as the kernels store it and the host cursor reads it
    double R[9], t[3];       // mRi, mti
    float Tcw[16];           // what iterate() makes of them: eye(4) with the float R and t
    int32_t N, pad;          // the candidate compute_pose chose: 1, 2 or 3
};
static_assert(sizeof(OrbxPnpHyp) == 168, "packed for the device");

enum { ORBX_PNP_SWEEPS = 30,            // sweep cap of both Jacobi routines
       ORBX_PNP_HYP_LANES = 32 };       // hypotheses (lanes) per workgroup of k_pnp_hypotheses
#define ORBX_PNP_JACOBI_EPS 1e-40       // cyclic Jacobi stops unless off > EPS * dia (sums of squares)
#define ORBX_PNP_SVD_EPS 1e-30          // one-sided Jacobi rotates a pair when gamma^2 > EPS * (alpha * beta)
#define ORBX_PNP_RANK_EPS 1e-9          // sigma_2 <= EPS * sigma_0: the third columns are completed by cross products

// workspace layout (doubles)
enum { ORBX_PNP_A = 0,                  // 12 x 12, row major: MtM (upper triangle) / PW0tPW0 as a 3 x 3 with row stride 3
       ORBX_PNP_V = 144,                // 12 x 12 eigenvectors as columns (3 x 3 with row stride 3)
       ORBX_PNP_MROW = 288,             // one row of M
       ORBX_PNP_L = 300,                // l_6x10
       ORBX_PNP_RHO = 360,              // 6
       ORBX_PNP_CWS = 366,              // 4 x 3
       ORBX_PNP_CCS = 378,              // 4 x 3
       ORBX_PNP_QA = 390,               // 6 x nc, nc <= 5
       ORBX_PNP_QB = 420,               // 6
       ORBX_PNP_QA1 = 426, ORBX_PNP_QA2 = 431, ORBX_PNP_QX = 436,   // 5 each
       ORBX_PNP_BETAS = 441,            // 4
       ORBX_PNP_G = 445,                // 3 x 3 ABt -> U
       ORBX_PNP_GV = 454,               // 3 x 3 V
       ORBX_PNP_GS = 463,               // 3 singular values
       ORBX_PNP_RT = 466,               // R (9) | t (3) of the candidate at hand
       ORBX_PNP_BEST = 478,             // R (9) | t (3) of the best candidate so far
       ORBX_PNP_PC0 = 490, ORBX_PNP_PW0 = 493,
       ORBX_PNP_FIXED = 496 };          // then pws [n][3] | us [n][2] | alphas [n][4] | pcs [n][3]
#define ORBX_PNP_WS_DOUBLES(n) (ORBX_PNP_FIXED + 12 * (n))

struct OrbxPnpWs {
    double *p;
    int stride;
    ORBX_HD double &operator()(int e) const { return p[(long long)e * stride]; }
};

// cvSVD(CV_SVD_U_T) of a symmetric d x d double matrix (d = 3 or 12), as this library fixes it: cyclic Jacobi.  Only the upper
// triangle of a (row stride d) is read and written.  A sweep visits (p, q), p < q, row by row; a pair with a_pq == 0 is skipped;
// otherwise theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c,
// h = t a_pq, a_pp -= h, a_qq += h, a_pq = 0, (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq) for every other r, and the
// same update on columns p, q of V (which starts as I).  Before every sweep: off = the sum of the squared entries above the
// diagonal (row by row), dia = the sum of the squared diagonal; the loop stops unless off > 1e-40 dia (a NaN stops it) and
// after ORBX_PNP_SWEEPS sweeps.  Then a selection sort puts the eigenvalues in descending order: position i takes the first
// largest of positions i .. d - 1 (strict >, so the lowest position wins a tie) by swapping diagonal entries and columns of V.
// Row r of the reference's ut is column r of V; the sign of a vector is left as computed.
ORBX_HD static inline void orbx_pnp_jacobi(const OrbxPnpWs &W, int d) {
    const int A = ORBX_PNP_A, V = ORBX_PNP_V;
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) W(V + i * d + j) = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < ORBX_PNP_SWEEPS; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int p = 0; p < d; ++p) {
            const double app = W(A + p * d + p);
            dia = dia + app * app;
            for (int q = p + 1; q < d; ++q) { const double x = W(A + p * d + q); off = off + x * x; }
        }
        if (!(off > ORBX_PNP_JACOBI_EPS * dia)) break;
        for (int p = 0; p < d - 1; ++p)
            for (int q = p + 1; q < d; ++q) {
                const double apq = W(A + p * d + q);
                if (apq != 0.0) {
                    const double app = W(A + p * d + p), aqq = W(A + q * d + q);
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double den = __builtin_fabs(theta) + sqrt(theta * theta + 1.0);
                    const double t = (theta < 0.0 ? -1.0 : 1.0) / den;
                    const double c = 1.0 / sqrt(t * t + 1.0);
                    const double s = t * c;
                    const double h = t * apq;
                    W(A + p * d + p) = app - h;
                    W(A + q * d + q) = aqq + h;
                    W(A + p * d + q) = 0.0;
                    for (int r = 0; r < d; ++r) {
                        if (r != p && r != q) {
                            const int ip = r < p ? A + r * d + p : A + p * d + r, iq = r < q ? A + r * d + q : A + q * d + r;
                            const double arp = W(ip), arq = W(iq);
                            W(ip) = c * arp - s * arq;
                            W(iq) = s * arp + c * arq;
                        }
                        const double vrp = W(V + r * d + p), vrq = W(V + r * d + q);
                        W(V + r * d + p) = c * vrp - s * vrq;
                        W(V + r * d + q) = s * vrp + c * vrq;
                    }
                }
            }
    }
    for (int i = 0; i < d - 1; ++i) {
        int m = i;
        double best = W(A + i * d + i);
        for (int j = i + 1; j < d; ++j) { const double x = W(A + j * d + j); if (x > best) { best = x; m = j; } }
        if (m != i) {
            W(A + m * d + m) = W(A + i * d + i);
            W(A + i * d + i) = best;
            for (int r = 0; r < d; ++r) { const double x = W(V + r * d + i); W(V + r * d + i) = W(V + r * d + m); W(V + r * d + m) = x; }
        }
    }
}

// PnPsolver::qr_solve (:1380-1514) for a 6 x nc system in QA / QB, operation by operation -- including its eta, which is the
// largest |a_ik| over i = k .. nr - 2 (the source reads the entry BEFORE it advances, so the last row never takes part).  The
// three cvSolve(CV_SVD) calls of find_betas_approx_* go through this routine too (F13).  Its singular branch (eta == 0) gives
// X = 0 (the source prints a message and leaves X as it was).
ORBX_HD static inline void orbx_pnp_qr_solve(const OrbxPnpWs &W, int nc) {
    const int nr = 6, A = ORBX_PNP_QA, B = ORBX_PNP_QB, A1 = ORBX_PNP_QA1, A2 = ORBX_PNP_QA2, X = ORBX_PNP_QX;
    for (int k = 0; k < nc; ++k) {
        double eta = __builtin_fabs(W(A + k * nc + k));
        for (int i = k + 1; i < nr; ++i) { const double elt = __builtin_fabs(W(A + (i - 1) * nc + k)); if (eta < elt) eta = elt; }
        if (eta == 0) {
            for (int i = 0; i < nc; ++i) W(X + i) = 0.0;
            return;
        }
        const double inv_eta = 1. / eta;
        double sum = 0.0;
        for (int i = k; i < nr; ++i) {
            const double x = W(A + i * nc + k) * inv_eta;
            W(A + i * nc + k) = x;
            sum = sum + x * x;
        }
        double sigma = sqrt(sum);
        if (W(A + k * nc + k) < 0) sigma = -sigma;
        const double akk = W(A + k * nc + k) + sigma;
        W(A + k * nc + k) = akk;
        const double a1k = sigma * akk;
        W(A1 + k) = a1k;
        W(A2 + k) = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            double sm = 0;
            for (int i = k; i < nr; ++i) sm = sm + W(A + i * nc + k) * W(A + i * nc + j);
            const double tau = sm / a1k;
            for (int i = k; i < nr; ++i) W(A + i * nc + j) = W(A + i * nc + j) - tau * W(A + i * nc + k);
        }
    }
    for (int j = 0; j < nc; ++j) {                 // b <- Qt b
        double tau = 0;
        for (int i = j; i < nr; ++i) tau = tau + W(A + i * nc + j) * W(B + i);
        tau = tau / W(A1 + j);
        for (int i = j; i < nr; ++i) W(B + i) = W(B + i) - tau * W(A + i * nc + j);
    }
    W(X + nc - 1) = W(B + nc - 1) / W(A2 + nc - 1);   // X = R-1 b
    for (int i = nc - 2; i >= 0; --i) {
        double sum = 0;
        for (int j = i + 1; j < nc; ++j) sum = sum + W(A + i * nc + j) * W(X + j);
        W(X + i) = (W(B + i) - sum) / W(A2 + i);
    }
}

// cvSolve(L_6xk, Rho, X, CV_SVD) as this library fixes it: qr_solve on the copied columns c0 .. of l_6x10
ORBX_HD static inline void orbx_pnp_lstsq(const OrbxPnpWs &W, int nc, int c0, int c1, int c2, int c3, int c4) {
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < nc; ++j) {
            const int c = j == 0 ? c0 : j == 1 ? c1 : j == 2 ? c2 : j == 3 ? c3 : c4;
            W(ORBX_PNP_QA + i * nc + j) = W(ORBX_PNP_L + 10 * i + c);
        }
        W(ORBX_PNP_QB + i) = W(ORBX_PNP_RHO + i);
    }
    orbx_pnp_qr_solve(W, nc);
}

// gauss_newton (:1338-1372): 5 rounds of compute_A_and_b_gauss_newton + qr_solve on ORBX_PNP_BETAS
ORBX_HD static inline void orbx_pnp_gauss_newton(const OrbxPnpWs &W) {
    for (int k = 0; k < 5; ++k) {
        const double b0 = W(ORBX_PNP_BETAS), b1 = W(ORBX_PNP_BETAS + 1), b2 = W(ORBX_PNP_BETAS + 2), b3 = W(ORBX_PNP_BETAS + 3);
        for (int i = 0; i < 6; ++i) {
            const int L = ORBX_PNP_L + 10 * i;
            const double l0 = W(L), l1 = W(L + 1), l2 = W(L + 2), l3 = W(L + 3), l4 = W(L + 4), l5 = W(L + 5), l6 = W(L + 6),
                         l7 = W(L + 7), l8 = W(L + 8), l9 = W(L + 9);
            W(ORBX_PNP_QA + 4 * i) = (((2 * l0) * b0 + l1 * b1) + l3 * b2) + l6 * b3;
            W(ORBX_PNP_QA + 4 * i + 1) = ((l1 * b0 + (2 * l2) * b1) + l4 * b2) + l7 * b3;
            W(ORBX_PNP_QA + 4 * i + 2) = ((l3 * b0 + l4 * b1) + (2 * l5) * b2) + l8 * b3;
            W(ORBX_PNP_QA + 4 * i + 3) = ((l6 * b0 + l7 * b1) + l8 * b2) + (2 * l9) * b3;
            W(ORBX_PNP_QB + i) = W(ORBX_PNP_RHO + i) -
                (((((((((((l0 * b0) * b0 + (l1 * b0) * b1) + (l2 * b1) * b1) + (l3 * b0) * b2) + (l4 * b1) * b2) + (l5 * b2) * b2) +
                     (l6 * b0) * b3) + (l7 * b1) * b3) + (l8 * b2) * b3) + (l9 * b3) * b3));
        }
        orbx_pnp_qr_solve(W, 4);
        W(ORBX_PNP_BETAS) = b0 + W(ORBX_PNP_QX);
        W(ORBX_PNP_BETAS + 1) = b1 + W(ORBX_PNP_QX + 1);
        W(ORBX_PNP_BETAS + 2) = b2 + W(ORBX_PNP_QX + 2);
        W(ORBX_PNP_BETAS + 3) = b3 + W(ORBX_PNP_QX + 3);
    }
}

// cvSVD of the general 3 x 3 ABt in ORBX_PNP_G, giving U (in G) and V (in GV), as this library fixes it: one-sided Jacobi.
// V starts as I.  A sweep visits the column pairs (0,1) (0,2) (1,2): alpha = sum_k g_kp^2, beta = sum_k g_kq^2,
// gamma = sum_k g_kp g_kq (k = 0, 1, 2 in order); the pair is rotated when gamma^2 > 1e-30 (alpha beta):
// zeta = (beta - alpha) / (2 gamma), t = sgn(zeta) / (|zeta| + sqrt(zeta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c,
// (g_kp, g_kq) = (c g_kp - s g_kq, s g_kp + c g_kq) and the same on V.  The loop ends after a sweep without a rotation and
// after ORBX_PNP_SWEEPS sweeps.  sigma_j = sqrt(sum_k g_kj^2); a selection sort (as in orbx_pnp_jacobi) orders them descending
// with their columns of G and V; u_j = g_j / sigma_j.  When sigma_2 <= 1e-9 sigma_0 (coplanar points: ABt has rank 2) the third
// columns are u_2 = u_0 x u_1 and v_2 = v_0 x v_1, which gives a proper rotation U V^T.
ORBX_HD static inline void orbx_pnp_svd3(const OrbxPnpWs &W) {
    const int G = ORBX_PNP_G, V = ORBX_PNP_GV, S = ORBX_PNP_GS;
    for (int i = 0; i < 9; ++i) W(V + i) = i % 4 == 0 ? 1.0 : 0.0;
    for (int sweep = 0; sweep < ORBX_PNP_SWEEPS; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double g0p = W(G + p), g1p = W(G + 3 + p), g2p = W(G + 6 + p), g0q = W(G + q), g1q = W(G + 3 + q), g2q = W(G + 6 + q);
                const double alpha = (g0p * g0p + g1p * g1p) + g2p * g2p;
                const double beta = (g0q * g0q + g1q * g1q) + g2q * g2q;
                const double gamma = (g0p * g0q + g1p * g1q) + g2p * g2q;
                if (gamma * gamma > ORBX_PNP_SVD_EPS * (alpha * beta)) {
                    rotated = true;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double den = __builtin_fabs(zeta) + sqrt(zeta * zeta + 1.0);
                    const double t = (zeta < 0.0 ? -1.0 : 1.0) / den;
                    const double c = 1.0 / sqrt(t * t + 1.0);
                    const double s = t * c;
                    for (int k = 0; k < 3; ++k) {
                        const double gp = W(G + 3 * k + p), gq = W(G + 3 * k + q);
                        W(G + 3 * k + p) = c * gp - s * gq;
                        W(G + 3 * k + q) = s * gp + c * gq;
                        const double vp = W(V + 3 * k + p), vq = W(V + 3 * k + q);
                        W(V + 3 * k + p) = c * vp - s * vq;
                        W(V + 3 * k + q) = s * vp + c * vq;
                    }
                }
            }
        if (!rotated) break;
    }
    for (int j = 0; j < 3; ++j) {
        const double a = W(G + j), b = W(G + 3 + j), c = W(G + 6 + j);
        W(S + j) = sqrt((a * a + b * b) + c * c);
    }
    for (int i = 0; i < 2; ++i) {
        int m = i;
        double best = W(S + i);
        for (int j = i + 1; j < 3; ++j) { const double x = W(S + j); if (x > best) { best = x; m = j; } }
        if (m != i) {
            W(S + m) = W(S + i);
            W(S + i) = best;
            for (int r = 0; r < 3; ++r) {
                double x = W(G + 3 * r + i); W(G + 3 * r + i) = W(G + 3 * r + m); W(G + 3 * r + m) = x;
                x = W(V + 3 * r + i); W(V + 3 * r + i) = W(V + 3 * r + m); W(V + 3 * r + m) = x;
            }
        }
    }
    const double s0 = W(S), s1 = W(S + 1), s2 = W(S + 2);
    for (int k = 0; k < 3; ++k) { W(G + 3 * k) = W(G + 3 * k) / s0; W(G + 3 * k + 1) = W(G + 3 * k + 1) / s1; }
    if (s2 <= ORBX_PNP_RANK_EPS * s0) {
        const double a0 = W(G), a1 = W(G + 3), a2 = W(G + 6), b0 = W(G + 1), b1 = W(G + 4), b2 = W(G + 7);
        W(G + 2) = a1 * b2 - a2 * b1; W(G + 5) = a2 * b0 - a0 * b2; W(G + 8) = a0 * b1 - a1 * b0;
        const double c0 = W(V), c1 = W(V + 3), c2 = W(V + 6), d0 = W(V + 1), d1 = W(V + 4), d2 = W(V + 7);
        W(V + 2) = c1 * d2 - c2 * d1; W(V + 5) = c2 * d0 - c0 * d2; W(V + 8) = c0 * d1 - c1 * d0;
    } else {
        for (int k = 0; k < 3; ++k) W(G + 3 * k + 2) = W(G + 3 * k + 2) / s2;
    }
}

// compute_R_and_t (:998-1013) for ORBX_PNP_BETAS: compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t into
// ORBX_PNP_RT, and the value of reprojection_error
ORBX_HD static inline double orbx_pnp_R_and_t(const OrbxPnpWs &W, int n, double fu, double fv, double uc, double vc) {
    const int PWS = ORBX_PNP_FIXED, US = PWS + 3 * n, AL = PWS + 5 * n, PCS = PWS + 9 * n;
    const int CCS = ORBX_PNP_CCS, RT = ORBX_PNP_RT, G = ORBX_PNP_G, GV = ORBX_PNP_GV, PC0 = ORBX_PNP_PC0, PW0 = ORBX_PNP_PW0;
    for (int i = 0; i < 12; ++i) W(CCS + i) = 0.0;                       // compute_ccs: v = ut + 12 * (11 - i) is column 11 - i of V
    for (int i = 0; i < 4; ++i) {
        const double b = W(ORBX_PNP_BETAS + i);
        for (int j = 0; j < 12; ++j) W(CCS + j) = W(CCS + j) + b * W(ORBX_PNP_V + j * 12 + (11 - i));
    }
    for (int i = 0; i < n; ++i) {                                        // compute_pcs
        const double a0 = W(AL + 4 * i), a1 = W(AL + 4 * i + 1), a2 = W(AL + 4 * i + 2), a3 = W(AL + 4 * i + 3);
        for (int j = 0; j < 3; ++j)
            W(PCS + 3 * i + j) = ((a0 * W(CCS + j) + a1 * W(CCS + 3 + j)) + a2 * W(CCS + 6 + j)) + a3 * W(CCS + 9 + j);
    }
    if (W(PCS + 2) < 0.0) {                                              // solve_for_sign
        for (int i = 0; i < 12; ++i) W(CCS + i) = -W(CCS + i);
        for (int i = 0; i < 3 * n; ++i) W(PCS + i) = -W(PCS + i);
    }
    // estimate_R_and_t
    for (int j = 0; j < 3; ++j) { W(PC0 + j) = 0.0; W(PW0 + j) = 0.0; }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < 3; ++j) { W(PC0 + j) = W(PC0 + j) + W(PCS + 3 * i + j); W(PW0 + j) = W(PW0 + j) + W(PWS + 3 * i + j); }
    for (int j = 0; j < 3; ++j) { W(PC0 + j) = W(PC0 + j) / n; W(PW0 + j) = W(PW0 + j) / n; }
    for (int j = 0; j < 9; ++j) W(G + j) = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < 3; ++j) {
            const double dc = W(PCS + 3 * i + j) - W(PC0 + j);
            for (int c = 0; c < 3; ++c) W(G + 3 * j + c) = W(G + 3 * j + c) + dc * (W(PWS + 3 * i + c) - W(PW0 + c));
        }
    orbx_pnp_svd3(W);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            W(RT + 3 * i + j) = (W(G + 3 * i) * W(GV + 3 * j) + W(G + 3 * i + 1) * W(GV + 3 * j + 1)) + W(G + 3 * i + 2) * W(GV + 3 * j + 2);
    {
        const double r00 = W(RT), r01 = W(RT + 1), r02 = W(RT + 2), r10 = W(RT + 3), r11 = W(RT + 4), r12 = W(RT + 5), r20 = W(RT + 6),
                     r21 = W(RT + 7), r22 = W(RT + 8);
        const double det = (((((r00 * r11) * r22 + (r01 * r12) * r20) + (r02 * r10) * r21) - (r02 * r11) * r20) - (r01 * r10) * r22) -
                           (r00 * r12) * r21;
        if (det < 0) { W(RT + 6) = -r20; W(RT + 7) = -r21; W(RT + 8) = -r22; }
    }
    for (int i = 0; i < 3; ++i)
        W(RT + 9 + i) = W(PC0 + i) - ((W(RT + 3 * i) * W(PW0) + W(RT + 3 * i + 1) * W(PW0 + 1)) + W(RT + 3 * i + 2) * W(PW0 + 2));
    // reprojection_error
    double sum2 = 0.0;
    for (int i = 0; i < n; ++i) {
        const double x = W(PWS + 3 * i), y = W(PWS + 3 * i + 1), z = W(PWS + 3 * i + 2);
        const double Xc = ((W(RT) * x + W(RT + 1) * y) + W(RT + 2) * z) + W(RT + 9);
        const double Yc = ((W(RT + 3) * x + W(RT + 4) * y) + W(RT + 5) * z) + W(RT + 10);
        const double inv_Zc = 1.0 / (((W(RT + 6) * x + W(RT + 7) * y) + W(RT + 8) * z) + W(RT + 11));
        const double ue = uc + (fu * Xc) * inv_Zc;
        const double ve = vc + (fv * Yc) * inv_Zc;
        const double du = W(US + 2 * i) - ue, dv = W(US + 2 * i + 1) - ve;
        sum2 = sum2 + sqrt(du * du + dv * dv);
    }
    return sum2 / n;
}

// compute_pose (:738-817) for the n correspondences already in the workspace (pws at ORBX_PNP_FIXED, us behind them; floats
// widened as add_correspondence does).  cam = fu, fv, uc, vc.  Rt receives R (9, row major) | t (3); returns the chosen N.
ORBX_HD static inline int orbx_pnp_compute_pose(const OrbxPnpWs &W, int n, const double *cam, double *Rt) {
    const int PWS = ORBX_PNP_FIXED, US = PWS + 3 * n, AL = PWS + 5 * n;
    const int A = ORBX_PNP_A, V = ORBX_PNP_V, CWS = ORBX_PNP_CWS, L = ORBX_PNP_L, BT = ORBX_PNP_BETAS, X = ORBX_PNP_QX;
    const double fu = cam[0], fv = cam[1], uc = cam[2], vc = cam[3];
    // choose_control_points
    for (int j = 0; j < 3; ++j) W(CWS + j) = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < 3; ++j) W(CWS + j) = W(CWS + j) + W(PWS + 3 * i + j);
    for (int j = 0; j < 3; ++j) W(CWS + j) = W(CWS + j) / n;
    for (int j = 0; j < 9; ++j) W(A + j) = 0.0;
    for (int i = 0; i < n; ++i)                                          // cvMulTransposed(PW0, ., 1): rows in ascending order
        for (int a = 0; a < 3; ++a) {
            const double da = W(PWS + 3 * i + a) - W(CWS + a);
            for (int b = a; b < 3; ++b) W(A + 3 * a + b) = W(A + 3 * a + b) + da * (W(PWS + 3 * i + b) - W(CWS + b));
        }
    orbx_pnp_jacobi(W, 3);
    for (int i = 1; i < 4; ++i) {
        const double k = sqrt(W(A + 4 * (i - 1)) / n);
        for (int j = 0; j < 3; ++j) W(CWS + 3 * i + j) = W(CWS + j) + k * W(V + 3 * j + (i - 1));
    }
    // compute_barycentric_coordinates; cvInvert(CC, CV_SVD) as this library fixes it: the adjugate over the determinant
    {
        const double c00 = W(CWS + 3) - W(CWS), c01 = W(CWS + 6) - W(CWS), c02 = W(CWS + 9) - W(CWS);
        const double c10 = W(CWS + 4) - W(CWS + 1), c11 = W(CWS + 7) - W(CWS + 1), c12 = W(CWS + 10) - W(CWS + 1);
        const double c20 = W(CWS + 5) - W(CWS + 2), c21 = W(CWS + 8) - W(CWS + 2), c22 = W(CWS + 11) - W(CWS + 2);
        const double k00 = c11 * c22 - c12 * c21, k01 = c10 * c22 - c12 * c20, k02 = c10 * c21 - c11 * c20;
        const double det = (c00 * k00 - c01 * k01) + c02 * k02;
        const double i00 = k00 / det, i01 = (c02 * c21 - c01 * c22) / det, i02 = (c01 * c12 - c02 * c11) / det;
        const double i10 = (c12 * c20 - c10 * c22) / det, i11 = (c00 * c22 - c02 * c20) / det, i12 = (c02 * c10 - c00 * c12) / det;
        const double i20 = k02 / det, i21 = (c01 * c20 - c00 * c21) / det, i22 = (c00 * c11 - c01 * c10) / det;
        for (int i = 0; i < n; ++i) {
            const double d0 = W(PWS + 3 * i) - W(CWS), d1 = W(PWS + 3 * i + 1) - W(CWS + 1), d2 = W(PWS + 3 * i + 2) - W(CWS + 2);
            const double a1 = (i00 * d0 + i01 * d1) + i02 * d2;
            const double a2 = (i10 * d0 + i11 * d1) + i12 * d2;
            const double a3 = (i20 * d0 + i21 * d1) + i22 * d2;
            W(AL + 4 * i + 1) = a1; W(AL + 4 * i + 2) = a2; W(AL + 4 * i + 3) = a3;
            W(AL + 4 * i) = ((1.0 - a1) - a2) - a3;
        }
    }
    // fill_M and cvMulTransposed(M, MtM, 1): the rows of M in ascending order, one at a time
    for (int j = 0; j < 144; ++j) W(A + j) = 0.0;
    for (int r = 0; r < 2 * n; ++r) {
        const int i = r >> 1;
        const double f = (r & 1) ? fv : fu, cu = (r & 1) ? vc - W(US + 2 * i + 1) : uc - W(US + 2 * i);
        for (int k = 0; k < 4; ++k) {
            const double as = W(AL + 4 * i + k);
            W(ORBX_PNP_MROW + 3 * k) = (r & 1) ? 0.0 : as * f;
            W(ORBX_PNP_MROW + 3 * k + 1) = (r & 1) ? as * f : 0.0;
            W(ORBX_PNP_MROW + 3 * k + 2) = as * cu;
        }
        for (int a = 0; a < 12; ++a) {
            const double ma = W(ORBX_PNP_MROW + a);
            for (int b = a; b < 12; ++b) W(A + 12 * a + b) = W(A + 12 * a + b) + ma * W(ORBX_PNP_MROW + b);
        }
    }
    orbx_pnp_jacobi(W, 12);
    // compute_L_6x10: v[i] = row 11 - i of ut = column 11 - i of V; dv[i][j] = v[i]^[a] - v[i]^[b], (a, b) = 01 02 03 12 13 23
    for (int j = 0; j < 6; ++j) {
        const int a = j < 3 ? 0 : j < 5 ? 1 : 2, b = j < 3 ? j + 1 : j < 5 ? j - 1 : 3;
        double dv[4][3];
ORBX_UNROLL
        for (int i = 0; i < 4; ++i)
ORBX_UNROLL
            for (int c = 0; c < 3; ++c) dv[i][c] = W(V + (3 * a + c) * 12 + (11 - i)) - W(V + (3 * b + c) * 12 + (11 - i));
#define ORBX_PNP_DOT(x, y) ((dv[x][0] * dv[y][0] + dv[x][1] * dv[y][1]) + dv[x][2] * dv[y][2])
        W(L + 10 * j) = ORBX_PNP_DOT(0, 0);
        W(L + 10 * j + 1) = 2.0 * ORBX_PNP_DOT(0, 1);
        W(L + 10 * j + 2) = ORBX_PNP_DOT(1, 1);
        W(L + 10 * j + 3) = 2.0 * ORBX_PNP_DOT(0, 2);
        W(L + 10 * j + 4) = 2.0 * ORBX_PNP_DOT(1, 2);
        W(L + 10 * j + 5) = ORBX_PNP_DOT(2, 2);
        W(L + 10 * j + 6) = 2.0 * ORBX_PNP_DOT(0, 3);
        W(L + 10 * j + 7) = 2.0 * ORBX_PNP_DOT(1, 3);
        W(L + 10 * j + 8) = 2.0 * ORBX_PNP_DOT(2, 3);
        W(L + 10 * j + 9) = ORBX_PNP_DOT(3, 3);
#undef ORBX_PNP_DOT
        // compute_rho: dist2(cws[a], cws[b])
        const double e0 = W(CWS + 3 * a) - W(CWS + 3 * b), e1 = W(CWS + 3 * a + 1) - W(CWS + 3 * b + 1), e2 = W(CWS + 3 * a + 2) - W(CWS + 3 * b + 2);
        W(ORBX_PNP_RHO + j) = (e0 * e0 + e1 * e1) + e2 * e2;
    }
    int N = 1;
    double best_err = 0.0;
    for (int cand = 1; cand <= 3; ++cand) {
        if (cand == 1) {                                                 // find_betas_approx_1
            orbx_pnp_lstsq(W, 4, 0, 1, 3, 6, 0);
            const double x0 = W(X), x1 = W(X + 1), x2 = W(X + 2), x3 = W(X + 3);
            if (x0 < 0) {
                const double b0 = sqrt(-x0);
                W(BT) = b0; W(BT + 1) = -x1 / b0; W(BT + 2) = -x2 / b0; W(BT + 3) = -x3 / b0;
            } else {
                const double b0 = sqrt(x0);
                W(BT) = b0; W(BT + 1) = x1 / b0; W(BT + 2) = x2 / b0; W(BT + 3) = x3 / b0;
            }
        } else {                                                         // find_betas_approx_2, find_betas_approx_3
            orbx_pnp_lstsq(W, cand == 2 ? 3 : 5, 0, 1, 2, 3, 4);
            const double x0 = W(X), x1 = W(X + 1), x2 = W(X + 2);
            double b0, b1;
            if (x0 < 0) { b0 = sqrt(-x0); b1 = (x2 < 0) ? sqrt(-x2) : 0.0; }
            else { b0 = sqrt(x0); b1 = (x2 > 0) ? sqrt(x2) : 0.0; }
            if (x1 < 0) b0 = -b0;
            W(BT) = b0; W(BT + 1) = b1;
            W(BT + 2) = cand == 3 ? W(X + 3) / b0 : 0.0;
            W(BT + 3) = 0.0;
        }
        orbx_pnp_gauss_newton(W);
        const double err = orbx_pnp_R_and_t(W, n, fu, fv, uc, vc);
        if (cand == 1 || err < best_err) {
            N = cand;
            best_err = err;
            for (int i = 0; i < 12; ++i) W(ORBX_PNP_BEST + i) = W(ORBX_PNP_RT + i);
        }
    }
    for (int i = 0; i < 12; ++i) Rt[i] = W(ORBX_PNP_BEST + i);
    return N;
}

// what iterate() / Refine() keep of a pose: the doubles, eye(4) with their float conversions, the chosen N; NaNs canonical
ORBX_HD static inline void orbx_pnp_store(const double *Rt, int N, OrbxPnpHyp &H) {
    for (int i = 0; i < 9; ++i) H.R[i] = orbx_canond(Rt[i]);
    for (int i = 0; i < 3; ++i) H.t[i] = orbx_canond(Rt[9 + i]);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) H.Tcw[4 * i + j] = orbx_canonf((float)Rt[3 * i + j]);
        H.Tcw[4 * i + 3] = orbx_canonf((float)Rt[9 + i]);
        H.Tcw[12 + i] = 0.0f;
    }
    H.Tcw[15] = 1.0f;
    H.N = N; H.pad = 0;
}

// CheckInliers (:444-481) for one correspondence, with the source's mixed widths: Xc, Yc = the double row sum stored as float,
// invZc = 1 / the double sum stored as float, ue = uc + fu * Xc * invZc in double, distX stored as float, error2 in float,
// strict <.  R (9) | t (3) as stored in the hypothesis.
ORBX_HD static inline bool orbx_pnp_inlier(const double *R, const double *t, const double *cam, float x, float y, float z, float u,
                                           float v, float max_err) {
    const float Xc = (float)((((R[0] * (double)x + R[1] * (double)y) + R[2] * (double)z)) + t[0]);
    const float Yc = (float)((((R[3] * (double)x + R[4] * (double)y) + R[5] * (double)z)) + t[1]);
    const float invZc = (float)(1 / ((((R[6] * (double)x + R[7] * (double)y) + R[8] * (double)z)) + t[2]));
    const double ue = cam[2] + (cam[0] * (double)Xc) * (double)invZc;
    const double ve = cam[3] + (cam[1] * (double)Yc) * (double)invZc;
    const float distX = (float)((double)u - ue);
    const float distY = (float)((double)v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < max_err;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side (orbx_pnp.cpp, HIP-free): validation, packing, the host path, the cursor.
enum { ORBX_PNP_PLANES = 6,         // per correspondence: P3Dw (3) | P2D (2) | max_err
       ORBX_PNP_WAVES = 4,          // waves (iterations) per workgroup of k_pnp_inliers
       ORBX_PNP_CHUNK = 512 };      // correspondences staged in LDS at a time (12 KiB)
struct DPnpProb {                   // one problem that launches, as the kernels read it
    int32_t n, iterations, nwords, pad;   // nwords = ceil(n / 64)
    int32_t iter_off;               // first hypothesis / count of the problem
    int32_t pts_off;                // first float of its ORBX_PNP_PLANES planes of n floats
    int32_t word_off;               // first mask word: [iterations][nwords]
    int32_t pad2;
    double cam[4];                  // fu, fv, uc, vc
};
static_assert(sizeof(DPnpProb) == 64, "packed for the device");
// sets: [total_hyps][4]; a group: ORBX_PNP_WAVES iterations of k_pnp_inliers; tally: the inlier counts
using DPnpArgs = DRansacArgs<DPnpProb, OrbxPnpHyp, int32_t>;
using OrbxPnpPlan = OrbxRansacPlan;
orbx_status orbx_pnp_plan(int nproblems, const orbx_pnp_problem *problems, OrbxPnpPlan &plan, const char **why);
void orbx_pnp_pack(const orbx_pnp_problem *problems, const OrbxPnpPlan &plan, uint8_t *dst);
// the host path: reads the packed block, writes the downloaded block's layout (hyp | masks | counts) into out
void orbx_pnp_host_run(const OrbxPnpPlan &plan, const uint8_t *in, uint8_t *out);

struct OrbxPnpRefined {             // Refine() of one best mask
    bool ok = false;                // mnRefinedInliers > mRansacMinInliers
    int32_t count = 0;
    std::vector<uint64_t> mask;
    OrbxPnpHyp hyp;
};
struct OrbxPnpSolver {              // one solver of a batch: its own copy of the problem, its stored iterations, iterate()'s state
    int32_t n = 0, min_inliers = 0, max_its = 0, nwords = 0;
    bool launches = false;          // false: n < min_inliers, nothing is ever computed
    double cam[4] = {0, 0, 0, 0};
    std::vector<float> planes;      // ORBX_PNP_PLANES planes of n floats, as packed
    std::vector<OrbxPnpHyp> hyp;    // the stored iterations: the batch call's, then the appended ones
    std::vector<int32_t> counts;
    std::vector<uint64_t> masks;    // [stored][nwords]
    int32_t done = 0, best_inliers = 0, best_it = -1;   // mnIterations, mnBestInliers, the iteration behind mvbBestInliers / mBestTcw
    int32_t refined_it = -1;        // the best mask `refined` belongs to
    OrbxPnpRefined refined;
};
struct orbx_pnp_batch {
    std::vector<OrbxPnpSolver> st;
};
// solvers with their copies of the problems, nothing stored yet; orbx_pnp_batch_take scatters a downloaded block into them
orbx_pnp_batch *orbx_pnp_batch_new(const orbx_pnp_problem *problems, const OrbxPnpPlan &plan);
void orbx_pnp_batch_take(orbx_pnp_batch *b, const OrbxPnpPlan &plan, const uint8_t *out);
// The cursor behind orbx_pnp_batch_iterate / _append / _best / _counts / _hypothesis; *why names what was wrong
int32_t orbx_pnp_cursor_iterate(orbx_pnp_batch *b, int k, int n_iterations, int32_t *no_more, uint8_t *inliers, int32_t *ninliers,
                                float *Tcw, const char **why);
orbx_status orbx_pnp_cursor_append(orbx_pnp_batch *b, int k, int nsets, const int32_t *sets, const char **why);
orbx_status orbx_pnp_cursor_best(const orbx_pnp_batch *b, int k, float *Tcw, int32_t *ninliers, int32_t *iteration, const char **why);
orbx_status orbx_pnp_cursor_counts(const orbx_pnp_batch *b, int k, int32_t *counts, int32_t *niterations, const char **why);
orbx_status orbx_pnp_cursor_hypothesis(const orbx_pnp_batch *b, int k, int iteration, double *Rt12, float *Tcw, int32_t *N,
                                       uint64_t *mask_words, const char **why);
