// orbx_sim3opt.h -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1383-1615) as scalar code shared by the host path
// (orbx_sim3opt.cpp) and the kernel (k_sim3_opt): what g2o executes for ONE free VertexSim3Expmap between fixed
// VertexSBAPointXYZ, with EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ edges whose Jacobians g2o takes numerically (central
// differences, delta = 1e-9), a dense 7x7 system and Levenberg-Marquardt.  tests/sim3opt_model.py restates it independently in
// numpy float64; DESIGN.md section 2 (F16) lists what was read from the reference and every arithmetic order this file fixes
// for itself where the reference leaves it to Eigen or libm.
//
// fp_mode: as in orbx_pose.h every expression is written operation by operation and the library is built with
// -ffp-contract=off; the only fused operations are the explicit ones inside orbx_pose_sincos and orbx_sim3opt_expd.  No exp, sin
// or cos of any math library is called.
#pragma once
#include "orbx_pose.h"     // orbx_lm.h, the quaternion helpers, orbx_pose_sincos
#include "orbx_ransac.h"   // orbx_canonf / orbx_canond, orbx_pad256

enum {
    ORBX_SIM3OPT_TERMS = 36,      // 28 of H (upper triangle row by row), 7 of b, rho0
    ORBX_SIM3OPT_NSIM = 15,       // the estimate and its 14 perturbations Sim3(+-delta e_d) * estimate
    ORBX_SIM3OPT_SIM = 16,        // doubles per entry of the table: the Sim3 (8) and its inverse (8)
    ORBX_SIM3OPT_PLANES = 12,     // x1c xyz, x2c xyz, obs1 uv, obs2 uv, invSigma2 1, invSigma2 2
    // k_sim3_opt's LDS in doubles: the [36][65] term array, the 36 broadcast sums and the table of the 15 Sim3
    ORBX_SIM3OPT_LDS_DOUBLES = ORBX_SIM3OPT_TERMS * 65 + ORBX_SIM3OPT_TERMS + ORBX_SIM3OPT_NSIM * ORBX_SIM3OPT_SIM
};
static_assert(ORBX_SIM3OPT_TERMS == OrbxLm<7>::TERMS, "the term layout of orbx_lm.h for 7 unknowns");
#define ORBX_SIM3OPT_DELTA 1e-9   // base_binary_edge.hpp:147

// g2o::Sim3: r (x, y, z, w) and t in q (never normalised), s
struct OrbxSim3 { OrbxPoseSE3 q; double s; };

// exp(x) for Sim3(Vector7d): k = round(x log2 e), r = x - k ln2 in two parts (the first product is exact), the Taylor
// polynomial of degree 13 on |r| <= ln2 / 2 by Horner, 2^k by its bits.  Only *, +, fma and int conversion.  NaN gives NaN;
// x > 709 is defined as +inf and x < -708 as 0 (no Sim3 update comes near either).
ORBX_HD static inline double orbx_sim3opt_expd(double x) {
    if (x != x) return x;
    if (x > 709.0) return __builtin_inf();
    if (x < -708.0) return 0.0;
    const double q = x * 0x1.71547652b82fep+0;
    const int k = (int)(q + (q < 0 ? -0.5 : 0.5));
    const double dk = -(double)k;
    double r = __builtin_fma(dk, 0x1.62e42feep-1, x);
    r = __builtin_fma(dk, 0x1.a39ef35793c76p-33, r);
    double p = 0x1.6124613a86d09p-33;                       // 1 / 13!
    p = __builtin_fma(r, p, 0x1.1eed8eff8d898p-29);         // 1 / 12!
    p = __builtin_fma(r, p, 0x1.ae64567f544e4p-26);         // 1 / 11!
    p = __builtin_fma(r, p, 0x1.27e4fb7789f5cp-22);         // 1 / 10!
    p = __builtin_fma(r, p, 0x1.71de3a556c734p-19);         // 1 / 9!
    p = __builtin_fma(r, p, 0x1.a01a01a01a01ap-16);         // 1 / 8!
    p = __builtin_fma(r, p, 0x1.a01a01a01a01ap-13);         // 1 / 7!
    p = __builtin_fma(r, p, 0x1.6c16c16c16c17p-10);         // 1 / 6!
    p = __builtin_fma(r, p, 0x1.1111111111111p-7);          // 1 / 5!
    p = __builtin_fma(r, p, 0x1.5555555555555p-5);          // 1 / 4!
    p = __builtin_fma(r, p, 0x1.5555555555555p-3);          // 1 / 3!
    p = __builtin_fma(r, p, 0.5);
    const double m = 1.0 + __builtin_fma(r * r, p, r);
    const uint64_t b = (uint64_t)(k + 1023) << 52;          // k in [-1022, 1023] for x in [-708, 709]
    double two_k;
    __builtin_memcpy(&two_k, &b, 8);
    return m * two_k;
}

// g2o::Sim3 gScm(toMatrix3d(R), toVector3d(t), s): floats widened, Quaterniond(R), nothing normalised
ORBX_HD static inline OrbxSim3 orbx_sim3opt_from_input(const float *R, const float *t, float s) {
    double m[9];
ORBX_UNROLL
    for (int i = 0; i < 9; ++i) m[i] = (double)R[i];
    OrbxSim3 S;
    orbx_pose_quat_from_R(m, S.q);
    S.q.tx = (double)t[0]; S.q.ty = (double)t[1]; S.q.tz = (double)t[2];
    S.s = (double)s;
    return S;
}
// Sim3::operator*: r = a.r * b.r (Eigen's product), t = a.s * (a.r * b.t) + a.t, s = a.s * b.s
ORBX_HD static inline OrbxSim3 orbx_sim3opt_mul(const OrbxSim3 &A, const OrbxSim3 &B) {
    const OrbxPoseSE3 &a = A.q, &b = B.q;
    OrbxSim3 R;
    double v[3];
    orbx_pose_rotate(a, b.tx, b.ty, b.tz, v);
    R.q.tx = A.s * v[0] + a.tx; R.q.ty = A.s * v[1] + a.ty; R.q.tz = A.s * v[2] + a.tz;
    R.q.qw = a.qw * b.qw - a.qx * b.qx - a.qy * b.qy - a.qz * b.qz;
    R.q.qx = a.qw * b.qx + a.qx * b.qw + a.qy * b.qz - a.qz * b.qy;
    R.q.qy = a.qw * b.qy + a.qy * b.qw + a.qz * b.qx - a.qx * b.qz;
    R.q.qz = a.qw * b.qz + a.qz * b.qw + a.qx * b.qy - a.qy * b.qx;
    R.s = A.s * B.s;
    return R;
}
// Sim3::inverse: (r*, r* ((-1 / s) t), 1 / s)
ORBX_HD static inline OrbxSim3 orbx_sim3opt_inverse(const OrbxSim3 &A) {
    OrbxSim3 R;
    R.q.qx = -A.q.qx; R.q.qy = -A.q.qy; R.q.qz = -A.q.qz; R.q.qw = A.q.qw;
    const double m = -1.0 / A.s;
    double v[3];
    orbx_pose_rotate(R.q, m * A.q.tx, m * A.q.ty, m * A.q.tz, v);
    R.q.tx = v[0]; R.q.ty = v[1]; R.q.tz = v[2];
    R.s = 1.0 / A.s;
    return R;
}
// Sim3(Vector7d update) (sim3.h:70-142), update = (omega, upsilon, sigma), all four eps branches.  3x3 products sum k = 0, 1,
// 2 in order; R = (I + a Omega) + b Omega^2; W = (A Omega + B Omega^2) + C I; t = W upsilon.
ORBX_HD static inline OrbxSim3 orbx_sim3opt_exp(const double *u) {
    const double o0 = u[0], o1 = u[1], o2 = u[2], sigma = u[6];
    const double theta = sqrt(o0 * o0 + o1 * o1 + o2 * o2);
    const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};
    double Om2[9], R[9], W[9];
    OrbxSim3 S;
    S.s = orbx_sim3opt_expd(sigma);
ORBX_UNROLL
    for (int i = 0; i < 3; ++i)
ORBX_UNROLL
        for (int j = 0; j < 3; ++j) Om2[3 * i + j] = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
    const double eps = 0.00001;
    const bool small_theta = theta < eps;
    double sn = 0.0, cs = 1.0, A, B, C;
    if (!small_theta) orbx_pose_sincos(theta, &sn, &cs);
    if (__builtin_fabs(sigma) < eps) {
        C = 1.0;
        if (small_theta) {
            A = 1.0 / 2.0;
            B = 1.0 / 6.0;
        } else {
            const double theta2 = theta * theta;
            A = (1.0 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1.0) / sigma;
        const double sigma2 = sigma * sigma;
        if (small_theta) {
            A = ((sigma - 1.0) * S.s + 1.0) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1.0) * S.s) / (sigma2 * sigma);
        } else {
            const double a = S.s * sn, b = S.s * cs;
            const double theta2 = theta * theta;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2;
        }
    }
    const double ra = small_theta ? 1.0 : sn / theta, rb = small_theta ? 1.0 : (1.0 - cs) / (theta * theta);
ORBX_UNROLL
    for (int i = 0; i < 9; ++i) {
        const double id = i % 4 == 0 ? 1.0 : 0.0;
        R[i] = small_theta ? (id + Om[i]) + Om2[i] : (id + ra * Om[i]) + rb * Om2[i];
        W[i] = (A * Om[i] + B * Om2[i]) + C * id;
    }
    orbx_pose_quat_from_R(R, S.q);
    S.q.tx = W[0] * u[3] + W[1] * u[4] + W[2] * u[5];
    S.q.ty = W[3] * u[3] + W[4] * u[4] + W[5] * u[5];
    S.q.tz = W[6] * u[3] + W[7] * u[4] + W[8] * u[5];
    return S;
}
// VertexSim3Expmap::oplusImpl: with _fix_scale update[6] is zeroed IN the caller's vector, then Sim3(update) * estimate
ORBX_HD static inline OrbxSim3 orbx_sim3opt_oplus(const OrbxSim3 &est, double *u, bool fix_scale) {
    if (fix_scale) u[6] = 0.0;
    return orbx_sim3opt_mul(orbx_sim3opt_exp(u), est);
}
// Entry idx of the table linearizeOplus() walks: 0 = the estimate, 1 + 2 d = oplus(+delta e_d), 2 + 2 d = oplus(-delta e_d);
// out[0..7] = the Sim3 (r x y z w, t, s), out[8..15] = its inverse.  The same for every edge, so built once per linearisation.
ORBX_HD static inline void orbx_sim3opt_store(const OrbxSim3 &S, double *o) {
    o[0] = S.q.qx; o[1] = S.q.qy; o[2] = S.q.qz; o[3] = S.q.qw; o[4] = S.q.tx; o[5] = S.q.ty; o[6] = S.q.tz; o[7] = S.s;
}
ORBX_HD static inline OrbxSim3 orbx_sim3opt_fetch(const double *o) {
    OrbxSim3 S;
    S.q.qx = o[0]; S.q.qy = o[1]; S.q.qz = o[2]; S.q.qw = o[3]; S.q.tx = o[4]; S.q.ty = o[5]; S.q.tz = o[6]; S.s = o[7];
    return S;
}
ORBX_HD static inline void orbx_sim3opt_table_entry(const OrbxSim3 &est, int idx, bool fix_scale, double *out) {
    OrbxSim3 P = est;
    if (idx > 0) {
        const int d = (idx - 1) >> 1;
        const double v = (idx - 1) & 1 ? -ORBX_SIM3OPT_DELTA : ORBX_SIM3OPT_DELTA;
        double u[7];
ORBX_UNROLL
        for (int k = 0; k < 7; ++k) u[k] = k == d ? v : 0.0;
        P = orbx_sim3opt_oplus(est, u, fix_scale);
    }
    orbx_sim3opt_store(P, out);
    orbx_sim3opt_store(orbx_sim3opt_inverse(P), out + 8);
}

struct OrbxSim3OptCam { double fx, fy, cx, cy; };
// One edge: the fixed point it maps (P2 for e12, P1 for e21), its observation and invSigma2, floats widened
struct OrbxSim3OptEdge { double X, Y, Z, ox, oy, w; };
// One problem's planes ([ORBX_SIM3OPT_PLANES][n] floats): host pointer on the host path, device pointer in the kernel
struct OrbxSim3OptView { const float *pl; int n; };
ORBX_HD static inline void orbx_sim3opt_load(const OrbxSim3OptView &v, int i, OrbxSim3OptEdge &e12, OrbxSim3OptEdge &e21) {
    const long long n = v.n;
    e12.X = (double)v.pl[3 * n + i]; e12.Y = (double)v.pl[4 * n + i]; e12.Z = (double)v.pl[5 * n + i];
    e12.ox = (double)v.pl[6 * n + i]; e12.oy = (double)v.pl[7 * n + i]; e12.w = (double)v.pl[10 * n + i];
    e21.X = (double)v.pl[i]; e21.Y = (double)v.pl[n + i]; e21.Z = (double)v.pl[2 * n + i];
    e21.ox = (double)v.pl[8 * n + i]; e21.oy = (double)v.pl[9 * n + i]; e21.w = (double)v.pl[11 * n + i];
}
// computeError + chi2 of one edge under the Sim3 stored at s8 (the estimate for e12, its inverse for e21):
// err = obs - cam_map(project(S.map(X))), map = s (r X) + t; chi2 = e . (Omega e), Omega = w I, summed in component order
ORBX_HD static inline double orbx_sim3opt_error(const double *s8, const OrbxSim3OptCam &K, const OrbxSim3OptEdge &e, double *err) {
    const OrbxSim3 S = orbx_sim3opt_fetch(s8);
    double p[3];
    orbx_pose_rotate(S.q, e.X, e.Y, e.Z, p);
    p[0] = S.s * p[0] + S.q.tx; p[1] = S.s * p[1] + S.q.ty; p[2] = S.s * p[2] + S.q.tz;
    err[0] = e.ox - ((p[0] / p[2]) * K.fx + K.cx);
    err[1] = e.oy - ((p[1] / p[2]) * K.fy + K.cy);
    return err[0] * (e.w * err[0]) + err[1] * (e.w * err[1]);
}
// One edge's 36 terms.  tab: the table of orbx_sim3opt_table_entry; inv = 0 for e12 (the Sim3), 8 for e21 (its inverse).
// Column d of the Jacobian = (1 / (2 delta)) * (err(+delta e_d) - err(-delta e_d)), as linearizeOplus() computes it.
// t[0..27] = A^T (rho1 Omega) A, upper triangle row by row; t[28..34] = A^T (rho1 (Omega e)); t[35] = rho0.  Per entry the rows
// are summed in order r = 0, 1; a product is (A_rj * W) * A_rk with W = rho1 * w, and A_rj * (rho1 * (w * e_r)) for b.
ORBX_HD static inline void orbx_sim3opt_terms(const double *tab, int inv, const OrbxSim3OptCam &K, const OrbxSim3OptEdge &e, double delta,
                                              double *t) {
    double err[2], ep[2], em[2], J0[7], J1[7], rho1;
    const double chi2 = orbx_sim3opt_error(tab + inv, K, e, err);
    t[35] = orbx_lm_huber(chi2, delta, &rho1);
    const double scalar = 1.0 / (2 * ORBX_SIM3OPT_DELTA);
ORBX_UNROLL
    for (int d = 0; d < 7; ++d) {
        orbx_sim3opt_error(tab + (1 + 2 * d) * ORBX_SIM3OPT_SIM + inv, K, e, ep);
        orbx_sim3opt_error(tab + (2 + 2 * d) * ORBX_SIM3OPT_SIM + inv, K, e, em);
        J0[d] = scalar * (ep[0] - em[0]);
        J1[d] = scalar * (ep[1] - em[1]);
    }
    const double W = rho1 * e.w;
    const double we0 = rho1 * (e.w * err[0]), we1 = rho1 * (e.w * err[1]);
    int n = 0;
ORBX_UNROLL
    for (int j = 0; j < 7; ++j)
ORBX_UNROLL
        for (int k = j; k < 7; ++k) t[n++] = (J0[j] * W) * J0[k] + (J1[j] * W) * J1[k];
ORBX_UNROLL
    for (int j = 0; j < 7; ++j) t[28 + j] = J0[j] * we0 + J1[j] * we1;
}

// g2oS12 and Converter::toCvMat(g2oS12) as the result stores them, with the four counts
ORBX_HD static inline void orbx_sim3opt_store_result(const OrbxSim3 &est, int nin, int nbad, int n, int written, orbx_sim3opt_result *out) {
    out->r[0] = orbx_canond(est.q.qx); out->r[1] = orbx_canond(est.q.qy); out->r[2] = orbx_canond(est.q.qz); out->r[3] = orbx_canond(est.q.qw);
    out->t[0] = orbx_canond(est.q.tx); out->t[1] = orbx_canond(est.q.ty); out->t[2] = orbx_canond(est.q.tz);
    out->s = orbx_canond(est.s);
    double m[9];                                               // Converter::toCvMat(g2o::Sim3): [s R | t] narrowed to float
    orbx_pose_R_from_quat(est.q, m);
ORBX_UNROLL
    for (int r = 0; r < 3; ++r)
ORBX_UNROLL
        for (int c = 0; c < 3; ++c) out->T12[4 * r + c] = orbx_canonf((float)(est.s * m[3 * r + c]));
    out->T12[3] = orbx_canonf((float)est.q.tx); out->T12[7] = orbx_canonf((float)est.q.ty); out->T12[11] = orbx_canonf((float)est.q.tz);
    out->T12[12] = 0.f; out->T12[13] = 0.f; out->T12[14] = 0.f; out->T12[15] = 1.f;
    out->ninliers = nin; out->nbad = nbad; out->ncorr = n; out->written = written;
}

// OptimizeSim3 from optimize(5) on (SparseOptimizer::optimize: orbx_lm_optimize).  Ev supplies the three passes over the live
// correspondences (edges e12_i, e21_i for i ascending) and the vertex; everything here is uniform over the lanes of a wave that
// run it side by side:
//   void system(S, acc[36])      the table at S, then computeActiveErrors + activeRobustChi2 + buildSystem, edge order
//   double chi(S)                computeActiveErrors + activeRobustChi2 at S
//   OrbxSim3 oplus(S, x[7])      orbx_sim3opt_oplus with the problem's fix_scale (zeroes x[6] under it, before `scale` reads it)
//   int  classify(Slast)         e12->chi2() > th2 || e21->chi2() > th2 on every live correspondence, errors as they stand at
//                                Slast; nulls the match; returns how many it nulled
// n = nCorrespondences.  Fills r, t, s, T12 and the four counts of *out.
template <class Ev>
ORBX_HD static inline void orbx_sim3opt_run(Ev &ev, const OrbxSim3 &init, int n, orbx_sim3opt_result *out) {
    OrbxSim3 est = init, last = init;
    int nbad = 0, nin = 0, written = 0;
    if (n > 0) {                                               // no edge: no active vertex, optimize() returns at once
        orbx_lm_optimize<7>(ev, 5, est, last);
        nbad = ev.classify(last);
    }
    if (n - nbad >= 10) {
        orbx_lm_optimize<7>(ev, nbad > 0 ? 10 : 5, est, last);
        nin = n - nbad - ev.classify(last);
        written = 1;
    } else {
        est = init;                                            // return 0 before g2oS12 = vSim3_recov->estimate()
    }
    orbx_sim3opt_store_result(est, nin, nbad, n, written, out);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side (orbx_sim3opt.cpp, HIP-free: tests/san_sim3opt.cpp builds it alone): validation, packing, the library's host path.
// One problem as the kernel reads it
struct DSim3OptProb {
    int32_t n, fix_scale;
    int64_t off;               // first correspondence among all problems': planes at 12 * off floats, keep at off bytes
    float cam1[4], cam2[4], R[9], t[3], s, th2;
    double last[8];            // orbx_debug_sim3opt_inlier_test: the Sim3 at which computeActiveErrors ran last
};
static_assert(sizeof(DSim3OptProb) == 168, "packed for the device");
static_assert(sizeof(orbx_sim3opt_result) == 144, "stored by the kernel as it is");
// k_sim3_opt: device pointers
struct DSim3OptArgs {
    const DSim3OptProb *prob;
    const float *pts;
    orbx_sim3opt_result *res;
    uint8_t *keep;
    int nproblems, inlier_test_only;
};
// Uploaded block (one copy): DSim3OptProb[nproblems] | planes.  Downloaded block: orbx_sim3opt_result[nproblems] | keep.
struct OrbxSim3OptPlan {
    int nproblems = 0;
    size_t total = 0;
    size_t o_prob = 0, o_pts = 0, in_bytes = 0, o_res = 0, o_keep = 0, out_bytes = 0;
};
// Everything the host can see, before any device work.  ORBX_OK / ORBX_BAD_ARGUMENT / ORBX_UNSUPPORTED; *why names the argument.
orbx_status orbx_sim3opt_plan(int nproblems, const orbx_sim3opt_problem *problems, const orbx_sim3opt_result *results,
                              const double *last, bool inlier_test, OrbxSim3OptPlan &plan, const char **why);
void orbx_sim3opt_pack(const orbx_sim3opt_problem *problems, const double *last, const OrbxSim3OptPlan &plan, uint8_t *dst);
// The host path over the packed block: the problems one after the other, results | keep into out
void orbx_sim3opt_host_run(const OrbxSim3OptPlan &plan, const uint8_t *in, bool inlier_test, uint8_t *out);
// Downloaded block -> the caller's results and keep rows (n bytes each)
void orbx_sim3opt_unpack(const orbx_sim3opt_problem *problems, const OrbxSim3OptPlan &plan, const uint8_t *out, orbx_sim3opt_result *results);
