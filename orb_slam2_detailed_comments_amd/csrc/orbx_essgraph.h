// orbx_essgraph.h -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1050-1358) as scalar code shared by the host path
// (orbx_essgraph.cpp) and the kernels (k_essential_graph, k_eg_correct_points): what g2o executes for VertexSim3Expmap keyframes
// joined by EdgeSim3 edges with identity information and no robust kernel -- the measurements Sji = Sjw * Swi, the error
// log(C * S_i * S_j^-1), the numeric Jacobians of BaseBinaryEdge::linearizeOplus (central differences, delta = 1e-9), the 7 x 7
// block-sparse normal equations over the free keyframes, a block L D L^T in the elimination order the plan fixes,
// Levenberg-Marquardt with setUserLambdaInit(1e-16) over 20 iterations, the recovery of Tiw = [R, t / s] and the correction of
// the map points through two Sim3.  tests/essgraph_model.py restates it independently in numpy float64; DESIGN.md section 2
// (F20) lists what was read from the reference and every arithmetic order this file fixes for itself where the reference
// leaves it to Eigen, to libm or to a sparse Cholesky.
//
// ONE ORDER PER SUM.  As in orbx_localba.h the work is cut into phases over independent items and orbx_eg_run is written
// against an executor Ex with each(n, f), sync() and lead(): a plain loop on the host, lanes striding over the items and a
// barrier in the kernel.  The control values (chi2, lambda, rho, ...) are the same in every lane, so every branch around a
// barrier is uniform.  Sums over a vertex's incident edges and over the edges / vertices of the problem take ORBX_EG_CHAINS
// interleaved chains (chain c adds entries c, c + 64, ...), whose partials are then added in order of c.
//
// fp_mode: every expression is written operation by operation and the library is built with -ffp-contract=off; the only fused
// operations are the explicit ones inside orbx_pose_sincos and orbx_sim3opt_expd.  No log, acos, sin or cos of a math library
// is called.  Both fp_modes give the same bits on the host and on the device.
#pragma once
#include <vector>
#include "orbx_sim3opt.h"  // OrbxSim3, orbx_sim3opt_mul / _inverse / _exp / _oplus, orbx_lm.h, orbx_pose.h, orbx_ransac.h
#include "orbx_sim3.h"     // orbx_sim3_atan2_pos

enum {
    ORBX_EG_CHAINS = 64,
    ORBX_EG_THREADS = 256,
    ORBX_EG_ITERS = 20,
    ORBX_EG_MAX_LBLOCKS = 32768,      // 7 x 7 blocks of L (diagonal ones included) per problem on the device: 2 x 12.25 MiB of workspace
    ORBX_EG_MAX_VERTICES = 1 << 20,
    ORBX_EG_MAX_EDGES = 1 << 22,      // 98 Jacobian doubles per edge stay inside 32-bit item counts
    ORBX_EG_MAX_POINTS = 1 << 28      // map points of one call
};
static_assert(ORBX_EG_MAX_LBLOCKS == ORBX_ESSGRAPH_MAX_LBLOCKS, "the cap include/orbx.h documents");
#define ORBX_EG_LAMBDA0 1e-16         // setUserLambdaInit(1e-16), src/Optimizer.cc:1066

// ---------------------------------------------------------------------------------------------------------------------------
// log(x) for Sim3::log: x = 2^k m with m in [sqrt(1/2), sqrt(2)], f = m - 1 (exact), s = f / (2 + f), log m = 2 atanh s =
// 2 s + s z P(z) with z = s^2 and P the series 2/3 + 2/5 z + ... + 2/23 z^10 by Horner (z <= 0.0295: the next term is below
// 2^-63 of the first), log x = k ln2_hi + (log m + k ln2_lo).  Only *, +, / and the bits of x.  x < 0 and NaN give NaN, 0 gives
// -inf, +inf gives +inf.
ORBX_HD static inline double orbx_eg_logd(double x) {
    if (!(x > 0.0)) return x == 0.0 ? -__builtin_inf() : 0.0 * __builtin_inf();
    if (!(x <= ORBX_DBL_MAX)) return x;
    int k = 0;
    if (x < 0x1p-1022) { x = x * 0x1p54; k = -54; }
    uint64_t b;
    __builtin_memcpy(&b, &x, 8);
    k += (int)(b >> 52) - 1023;
    b = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m;
    __builtin_memcpy(&m, &b, 8);
    if (m > 0x1.6a09e667f3bcdp+0) { m = m * 0.5; k += 1; }
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double p = 2.0 / 23.0;
    p = p * z + 2.0 / 21.0;
    p = p * z + 2.0 / 19.0;
    p = p * z + 2.0 / 17.0;
    p = p * z + 2.0 / 15.0;
    p = p * z + 2.0 / 13.0;
    p = p * z + 2.0 / 11.0;
    p = p * z + 2.0 / 9.0;
    p = p * z + 2.0 / 7.0;
    p = p * z + 2.0 / 5.0;
    p = p * z + 2.0 / 3.0;
    const double lm = 2.0 * s + (s * z) * p;
    const double dk = (double)k;
    return dk * 0x1.62e42feep-1 + (lm + dk * 0x1.a39ef35793c76p-33);
}
// acos(d) of Sim3::log as this library fixes it: atan2(sqrt(1 - d d), d) by F12's routine; sq = sqrt(1 - d d), which the
// reference computes a second time for omega
ORBX_HD static inline double orbx_eg_theta(double d, double sq) { return orbx_sim3_atan2_pos(sq, d); }

// W.lu().solve(t) for the 3 x 3 of Sim3::log: Gaussian elimination of [W | t] with partial pivoting, the FIRST row of largest
// |pivot| (a NaN never wins), then back substitution; M is [3][4] row major and is destroyed
ORBX_HD static inline void orbx_eg_solve3(double *M, double *x) {
    {
        const double a0 = __builtin_fabs(M[0]), a1 = __builtin_fabs(M[4]), a2 = __builtin_fabs(M[8]);
        int p = 0;
        double best = a0;
        if (a1 > best) { p = 1; best = a1; }
        if (a2 > best) p = 2;
ORBX_UNROLL
        for (int j = 0; j < 4; ++j) {
            const double r0 = M[j], r1 = M[4 + j], r2 = M[8 + j];
            M[j] = p == 0 ? r0 : p == 1 ? r1 : r2;
            M[4 + j] = p == 1 ? r0 : r1;
            M[8 + j] = p == 2 ? r0 : r2;
        }
    }
    const double l1 = M[4] / M[0], l2 = M[8] / M[0];
ORBX_UNROLL
    for (int j = 1; j < 4; ++j) { M[4 + j] = M[4 + j] - l1 * M[j]; M[8 + j] = M[8 + j] - l2 * M[j]; }
    if (__builtin_fabs(M[9]) > __builtin_fabs(M[5])) {
ORBX_UNROLL
        for (int j = 1; j < 4; ++j) { const double r = M[4 + j]; M[4 + j] = M[8 + j]; M[8 + j] = r; }
    }
    const double l = M[9] / M[5];
    M[10] = M[10] - l * M[6];
    M[11] = M[11] - l * M[7];
    x[2] = M[11] / M[10];
    x[1] = (M[7] - M[6] * x[2]) / M[5];
    x[0] = ((M[3] - M[1] * x[1]) - M[2] * x[2]) / M[0];
}

// Sim3::log (sim3.h:148-230): res = (omega, upsilon, sigma), all four eps branches.  R = r.toRotationMatrix() of the quaternion
// as it stands (g2o::Sim3 never normalises it); deltaR = (R21 - R12, R02 - R20, R10 - R01); Omega^2 sums k = 0, 1, 2 in order;
// W = (A Omega + B Omega^2) + C I.
ORBX_HD static inline void orbx_eg_log(const OrbxSim3 &S, double *res) {
    const double sigma = orbx_eg_logd(S.s);
    double R[9];
    orbx_pose_R_from_quat(S.q, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double dr0 = R[7] - R[5], dr1 = R[2] - R[6], dr2 = R[3] - R[1];
    const double eps = 0.00001;
    const bool near = d > 1.0 - eps;
    double theta = 0.0, f = 0.5;
    if (!near) {
        const double sq = sqrt(1.0 - d * d);
        theta = orbx_eg_theta(d, sq);
        f = theta / (2.0 * sq);
    }
    const double o0 = f * dr0, o1 = f * dr1, o2 = f * dr2;
    double A, B, C;
    if (__builtin_fabs(sigma) < eps) {
        C = 1.0;
        if (near) {
            A = 1.0 / 2.0;
            B = 1.0 / 6.0;
        } else {
            double sn, cs;
            orbx_pose_sincos(theta, &sn, &cs);
            const double theta2 = theta * theta;
            A = (1.0 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1.0) / sigma;
        if (near) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * S.s + 1.0) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1.0) * S.s) / (sigma2 * sigma);
        } else {
            double sn, cs;
            orbx_pose_sincos(theta, &sn, &cs);
            const double theta2 = theta * theta;
            const double a = S.s * sn, b = S.s * cs;
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2;
        }
    }
    const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};
    double M[12];
ORBX_UNROLL
    for (int i = 0; i < 3; ++i)
ORBX_UNROLL
        for (int j = 0; j < 3; ++j) {
            const double om2 = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
            M[4 * i + j] = (A * Om[3 * i + j] + B * om2) + C * (i == j ? 1.0 : 0.0);
        }
    M[3] = S.q.tx; M[7] = S.q.ty; M[11] = S.q.tz;
    orbx_eg_solve3(M, res + 3);
    res[0] = o0; res[1] = o1; res[2] = o2;
    res[6] = sigma;
}

// ---------------------------------------------------------------------------------------------------------------------------
// One problem as the kernels read it: the counts and where its three blocks start (bytes from the call's input, workspace and
// output blocks).  Every array inside a block follows from the counts (orbx_eg_bind).
struct DEgProb {
    int32_t nv, ne, nact, nblk, npair, naent, ninc, nrounds, fix_scale, npoints;
    int64_t o_in, o_work, o_out;
    int64_t pt_begin;               // the problem's first point among the call's
};
static_assert(sizeof(DEgProb) == 72, "packed for the device");
struct DEgArgs {                    // k_essential_graph, k_eg_correct_points: device pointers
    const DEgProb *prob;
    const uint8_t *in;
    uint8_t *work, *out;
    int nproblems;                  // the results stand at the start of out
    int64_t npoints;                // of the call
    int64_t o_pts_in, o_pts_out;    // world [3] float | ref int32 | problem int32 per point in `in`; world_out in `out`
};

struct OrbxEgCtx {
    int nv, ne, nact, nblk, npair, naent, ninc, nrounds, fix_scale;
    // input block
    const double *Scw;              // [nv][8] r x y z w, t, s
    const double *Snc;              // [nv][8] NonCorrected where present, else Scw
    const int32_t *edges;           // [ne][3] i, j, kind (1: loop connection, both poses from Scw)
    const int32_t *acol;            // [nv] column (position in the elimination order) of an active vertex, -1: fixed or without edge
    const int32_t *col_vertex;      // [nact]
    const int32_t *inc_begin;       // [nact + 1] incident edges by column,
    const int32_t *inc;             // [ninc]     2 * edge + side, ascending
    const int32_t *round_begin;     // [nrounds + 1] columns by round
    const int32_t *blk_begin;       // [nact + 1] blocks of L by column: the diagonal one first, then rows ascending
    const int32_t *blk_ij;          // [nblk][2] row column, column column
    const int32_t *pair_begin;      // [nblk + 1]
    const int32_t *pair;            // [npair][2] block L(i, k), block L(j, k), k ascending
    const int32_t *aent_begin;      // [nblk + 1] an off-diagonal block's edges,
    const int32_t *aent;            // [naent]    2 * edge + side of the ROW vertex, ascending
    const int32_t *row_begin;       // [nact + 1] off-diagonal blocks by row,
    const int32_t *row_blk;         // [nblk - nact] column ascending
    // workspace
    OrbxSim3 *est, *bak;            // [nv]
    double *meas;                   // [ne][8]
    double *err, *echi;             // [ne][7], [ne]
    double *J;                      // [ne][2][7][7]: side, column d, component
    double *Ab, *Lb;                // [nblk][49] row major: H, then T and L in place
    double *bv, *dd, *y, *x;        // [7 nact]
    double *red;                    // [64]
    int32_t *iw;                    // [4]
    // output block
    double *Siw_out;                // [nv][8]
    float *Tiw_out;                 // [nv][16]
};
struct OrbxEgCarve {
    uint8_t *base; size_t off;
    template <class T> ORBX_HD T *take(size_t n) {
        off = (off + 7) & ~(size_t)7;
        T *p = (T *)(base + off);
        off += n * sizeof(T);
        return p;
    }
};
struct OrbxEgSizes { size_t in_bytes, work_bytes, out_bytes; };
ORBX_HD static inline OrbxEgSizes orbx_eg_bind(const DEgProb &P, const uint8_t *in, uint8_t *work, uint8_t *out, OrbxEgCtx &c) {
    c.nv = P.nv; c.ne = P.ne; c.nact = P.nact; c.nblk = P.nblk; c.npair = P.npair; c.naent = P.naent; c.ninc = P.ninc;
    c.nrounds = P.nrounds; c.fix_scale = P.fix_scale;
    const size_t nv = (size_t)P.nv, ne = (size_t)P.ne, na = (size_t)P.nact, nb = (size_t)P.nblk;
    OrbxEgSizes s;
    OrbxEgCarve a = {(uint8_t *)in, 0};
    c.Scw = a.take<double>(8 * nv); c.Snc = a.take<double>(8 * nv); c.edges = a.take<int32_t>(3 * ne); c.acol = a.take<int32_t>(nv);
    c.col_vertex = a.take<int32_t>(na); c.inc_begin = a.take<int32_t>(na + 1); c.inc = a.take<int32_t>((size_t)P.ninc);
    c.round_begin = a.take<int32_t>((size_t)P.nrounds + 1); c.blk_begin = a.take<int32_t>(na + 1); c.blk_ij = a.take<int32_t>(2 * nb);
    c.pair_begin = a.take<int32_t>(nb + 1); c.pair = a.take<int32_t>(2 * (size_t)P.npair);
    c.aent_begin = a.take<int32_t>(nb + 1); c.aent = a.take<int32_t>((size_t)P.naent);
    c.row_begin = a.take<int32_t>(na + 1); c.row_blk = a.take<int32_t>(nb - na);
    s.in_bytes = (a.off + 255) & ~(size_t)255;
    OrbxEgCarve b = {work, 0};
    c.est = b.take<OrbxSim3>(nv); c.bak = b.take<OrbxSim3>(nv); c.meas = b.take<double>(8 * ne);
    c.err = b.take<double>(7 * ne); c.echi = b.take<double>(ne); c.J = b.take<double>(98 * ne);
    c.Ab = b.take<double>(49 * nb); c.Lb = b.take<double>(49 * nb);
    c.bv = b.take<double>(7 * na); c.dd = b.take<double>(7 * na); c.y = b.take<double>(7 * na); c.x = b.take<double>(7 * na);
    c.red = b.take<double>(ORBX_EG_CHAINS); c.iw = b.take<int32_t>(4);
    s.work_bytes = (b.off + 255) & ~(size_t)255;
    OrbxEgCarve o = {out, 0};
    c.Siw_out = o.take<double>(8 * nv); c.Tiw_out = o.take<float>(16 * nv);
    s.out_bytes = (o.off + 255) & ~(size_t)255;
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// EdgeSim3::computeError: log((C * S_i) * S_j^-1)
ORBX_HD static inline void orbx_eg_error(const OrbxSim3 &C, const OrbxSim3 &Si, const OrbxSim3 &Sj, double *err) {
    orbx_eg_log(orbx_sim3opt_mul(orbx_sim3opt_mul(C, Si), orbx_sim3opt_inverse(Sj)), err);
}
// an edge is active unless both its vertices are fixed (allVerticesFixed, sparse_optimizer.cpp:234)
ORBX_HD static inline bool orbx_eg_edge_active(const OrbxEgCtx &c, int e) {
    return c.acol[c.edges[3 * e]] >= 0 || c.acol[c.edges[3 * e + 1]] >= 0;
}
// computeError + chi2 = e . (I e) of edge e at the current estimates, components in order
ORBX_HD static inline void orbx_eg_edge_error(const OrbxEgCtx &c, int e) {
    double *err = c.err + 7 * (size_t)e;
    if (!orbx_eg_edge_active(c, e)) {
ORBX_UNROLL
        for (int k = 0; k < 7; ++k) err[k] = 0.0;
        c.echi[e] = 0.0;
        return;
    }
    double v[7];
    orbx_eg_error(orbx_sim3opt_fetch(c.meas + 8 * (size_t)e), c.est[c.edges[3 * e]], c.est[c.edges[3 * e + 1]], v);
    double s = v[0] * v[0];
ORBX_UNROLL
    for (int k = 1; k < 7; ++k) s = s + v[k] * v[k];
ORBX_UNROLL
    for (int k = 0; k < 7; ++k) err[k] = v[k];
    c.echi[e] = s;
}
// BaseBinaryEdge::linearizeOplus, one column: side 0 perturbs vertex i, side 1 vertex j; column d = (1 / (2 delta)) *
// (err(oplus(+delta e_d)) - err(oplus(-delta e_d))).  A fixed vertex has no Jacobian.
ORBX_HD static inline void orbx_eg_jacobian_column(const OrbxEgCtx &c, int e, int side, int d) {
    if (c.acol[c.edges[3 * e + side]] < 0) return;
    const OrbxSim3 C = orbx_sim3opt_fetch(c.meas + 8 * (size_t)e);
    const OrbxSim3 Si = c.est[c.edges[3 * e]], Sj = c.est[c.edges[3 * e + 1]];
    const double scalar = 1.0 / (2 * ORBX_SIM3OPT_DELTA);
    double u[7], ep[7], em[7];
ORBX_UNROLL
    for (int k = 0; k < 7; ++k) u[k] = k == d ? ORBX_SIM3OPT_DELTA : 0.0;
    const OrbxSim3 Pp = orbx_sim3opt_oplus(side ? Sj : Si, u, c.fix_scale != 0);
ORBX_UNROLL
    for (int k = 0; k < 7; ++k) u[k] = k == d ? -ORBX_SIM3OPT_DELTA : 0.0;
    const OrbxSim3 Pm = orbx_sim3opt_oplus(side ? Sj : Si, u, c.fix_scale != 0);
    if (side) { orbx_eg_error(C, Si, Pp, ep); orbx_eg_error(C, Si, Pm, em); }
    else { orbx_eg_error(C, Pp, Sj, ep); orbx_eg_error(C, Pm, Sj, em); }
    double *col = c.J + 98 * (size_t)e + 49 * side + 7 * d;
ORBX_UNROLL
    for (int k = 0; k < 7; ++k) col[k] = scalar * (ep[k] - em[k]);
}
// a . b over the 7 components in order
ORBX_HD static inline double orbx_eg_dot7(const double *a, const double *b) {
    double s = a[0] * b[0];
ORBX_UNROLL
    for (int k = 1; k < 7; ++k) s = s + a[k] * b[k];
    return s;
}

// The partials in c.red added in order of the chain; every lane gets the same value
template <class Ex> ORBX_HD static inline double orbx_eg_sum64(Ex &ex, const OrbxEgCtx &c) {
    double s = 0.0;
    for (int k = 0; k < ORBX_EG_CHAINS; ++k) s = s + c.red[k];
    ex.sync();
    return s;
}
// activeChi2 from the edges' shares
template <class Ex> ORBX_HD static inline double orbx_eg_chi_total(Ex &ex, const OrbxEgCtx &c) {
    ex.each(ORBX_EG_CHAINS, [&](int ch) {
        double s = 0.0;
        for (int e = ch; e < c.ne; e += ORBX_EG_CHAINS) s = s + c.echi[e];
        c.red[ch] = s;
    });
    return orbx_eg_sum64(ex, c);
}
// computeActiveErrors + activeChi2 at the current estimates
template <class Ex> ORBX_HD static inline double orbx_eg_chi(Ex &ex, const OrbxEgCtx &c) {
    ex.each(c.ne, [&](int e) { orbx_eg_edge_error(c, e); });
    return orbx_eg_chi_total(ex, c);
}
// computeActiveErrors + activeChi2 + linearizeOplus + buildSystem at the current estimates.  One item per (edge, side, column)
// and one per edge's error; then one item per (block, row): a diagonal block's row r is sum over the vertex's incident edges of
// (J col r) . (J col c), c = 0..6, in 64 chains; an off-diagonal block's row r is sum over its edges of (J_row col r) . (J_col
// col c), edges ascending; one item per (column, r) for b = -sum (J col r) . e, in 64 chains.  Returns the chi2.
template <class Ex> ORBX_HD static inline double orbx_eg_system(Ex &ex, const OrbxEgCtx &c) {
    ex.each(c.ne * 15, [&](int idx) {
        const int e = idx / 15, k = idx % 15;
        if (k == 14) { orbx_eg_edge_error(c, e); return; }
        if (!orbx_eg_edge_active(c, e)) return;
        orbx_eg_jacobian_column(c, e, k / 7, k % 7);
    });
    ex.each((c.nblk + c.nact) * 7, [&](int idx) {
        const int b = idx / 7, r = idx % 7;
        if (b >= c.nblk) {                                     // b_(column)[r]
            const int col = b - c.nblk;
            double s = 0.0;
            for (int ch = 0; ch < ORBX_EG_CHAINS; ++ch) {
                if (c.inc_begin[col] + ch >= c.inc_begin[col + 1]) break;   // (an empty chain adds +0: nothing)
                double p = 0.0;
                for (int k = c.inc_begin[col] + ch; k < c.inc_begin[col + 1]; k += ORBX_EG_CHAINS) {
                    const int es = c.inc[k];
                    p = p - orbx_eg_dot7(c.J + 49 * (size_t)es + 7 * r, c.err + 7 * (size_t)(es >> 1));
                }
                s = s + p;
            }
            c.bv[7 * col + r] = s;
            return;
        }
        double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const int bi = c.blk_ij[2 * b], bj = c.blk_ij[2 * b + 1];
        if (bi == bj) {
            for (int ch = 0; ch < ORBX_EG_CHAINS; ++ch) {
                if (c.inc_begin[bj] + ch >= c.inc_begin[bj + 1]) break;
                double p[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (int k = c.inc_begin[bj] + ch; k < c.inc_begin[bj + 1]; k += ORBX_EG_CHAINS) {
                    const double *Jv = c.J + 49 * (size_t)c.inc[k];
ORBX_UNROLL
                    for (int cc = 0; cc < 7; ++cc) p[cc] = p[cc] + orbx_eg_dot7(Jv + 7 * r, Jv + 7 * cc);
                }
ORBX_UNROLL
                for (int cc = 0; cc < 7; ++cc) acc[cc] = acc[cc] + p[cc];
            }
        } else {
            for (int k = c.aent_begin[b]; k < c.aent_begin[b + 1]; ++k) {
                const int es = c.aent[k];
                const double *Jr = c.J + 49 * (size_t)es, *Jc = c.J + 49 * (size_t)(es ^ 1);
ORBX_UNROLL
                for (int cc = 0; cc < 7; ++cc) acc[cc] = acc[cc] + orbx_eg_dot7(Jr + 7 * r, Jc + 7 * cc);
            }
        }
ORBX_UNROLL
        for (int cc = 0; cc < 7; ++cc) c.Ab[49 * (size_t)b + 7 * r + cc] = acc[cc];
    });
    return orbx_eg_chi_total(ex, c);
}
// computeScale over the whole x: sum x_j (lambda x_j + b_j), chains over the columns
template <class Ex> ORBX_HD static inline double orbx_eg_scale(Ex &ex, const OrbxEgCtx &c, double lambda) {
    ex.each(ORBX_EG_CHAINS, [&](int ch) {
        double s = 0.0;
        for (int col = ch; col < c.nact; col += ORBX_EG_CHAINS)
            for (int j = 0; j < 7; ++j) { const double xv = c.x[7 * col + j]; s = s + xv * (lambda * xv + c.bv[7 * col + j]); }
        c.red[ch] = s;
    });
    return orbx_eg_sum64(ex, c);
}

// (H + lambda I) x = b by the block L D L^T, round by round.  Per round: T(i, j) = A(i, j) + [i = j] lambda I - sum_k (L(i, k)
// D_k) L(j, k)^T, one item per (block, row), k in the order of the block's pair list; the unpivoted 7 x 7 L D L^T of T(j, j), one
// item per column (orbx_lm_solve's recurrences, in place); L(i, j) = T(i, j) L_jj^-T D_j^-1, one item per (block, row).  The
// system counts as positive when every pivot is > 0 and finite; otherwise x = 0.  Forward solve per column, rounds ascending;
// backward solve per column, rounds descending.
template <class Ex> ORBX_HD static inline bool orbx_eg_solve(Ex &ex, const OrbxEgCtx &c, double lambda) {
    for (int rd = 0; rd < c.nrounds; ++rd) {
        const int c0 = c.round_begin[rd], c1 = c.round_begin[rd + 1];
        const int b0 = c.blk_begin[c0], b1 = c.blk_begin[c1];
        ex.each((b1 - b0) * 7, [&](int idx) {
            const int b = b0 + idx / 7, r = idx % 7;
            const bool diag = c.blk_ij[2 * b] == c.blk_ij[2 * b + 1];
            double acc[7];
ORBX_UNROLL
            for (int cc = 0; cc < 7; ++cc) {
                const double v = c.Ab[49 * (size_t)b + 7 * r + cc];
                acc[cc] = diag && cc == r ? v + lambda : v;
            }
            for (int k = c.pair_begin[b]; k < c.pair_begin[b + 1]; ++k) {
                const int pa = c.pair[2 * k], pb = c.pair[2 * k + 1];
                const double *Li = c.Lb + 49 * (size_t)pa + 7 * r, *Lj = c.Lb + 49 * (size_t)pb;
                const double *dk = c.dd + 7 * c.blk_ij[2 * pa + 1];
                double w[7];
ORBX_UNROLL
                for (int m = 0; m < 7; ++m) w[m] = Li[m] * dk[m];
ORBX_UNROLL
                for (int cc = 0; cc < 7; ++cc) acc[cc] = acc[cc] - orbx_eg_dot7(w, Lj + 7 * cc);
            }
ORBX_UNROLL
            for (int cc = 0; cc < 7; ++cc) c.Lb[49 * (size_t)b + 7 * r + cc] = acc[cc];
        });
        ex.each(c1 - c0, [&](int idx) {
            const int col = c0 + idx;
            double *M = c.Lb + 49 * (size_t)c.blk_begin[col], *d = c.dd + 7 * col;
            for (int j = 0; j < 7; ++j) {
                double s = M[7 * j + j];
                for (int k = 0; k < j; ++k) s = s - M[7 * j + k] * (M[7 * j + k] * d[k]);
                d[j] = s;
                for (int i = j + 1; i < 7; ++i) {
                    double t = M[7 * i + j];
                    for (int k = 0; k < j; ++k) t = t - M[7 * i + k] * (M[7 * j + k] * d[k]);
                    M[7 * i + j] = t / s;
                }
            }
        });
        ex.each((b1 - b0) * 7, [&](int idx) {
            const int b = b0 + idx / 7, r = idx % 7;
            const int col = c.blk_ij[2 * b + 1];
            if (c.blk_ij[2 * b] == col) return;
            double *row = c.Lb + 49 * (size_t)b + 7 * r;
            const double *Ljj = c.Lb + 49 * (size_t)c.blk_begin[col], *d = c.dd + 7 * col;
            for (int cc = 0; cc < 7; ++cc) {
                double t = row[cc];
                for (int m = 0; m < cc; ++m) t = t - (row[m] * d[m]) * Ljj[7 * cc + m];
                row[cc] = t / d[cc];
            }
        });
    }
    ex.each(1, [&](int) { c.iw[0] = 1; });
    ex.each(7 * c.nact, [&](int i) { if (!(c.dd[i] > 0 && c.dd[i] <= ORBX_DBL_MAX)) c.iw[0] = 0; });
    const bool ok = c.iw[0] != 0;
    ex.sync();
    if (!ok) {
        ex.each(7 * c.nact, [&](int i) { c.x[i] = 0.0; });
        return false;
    }
    // L y = b: y_j = L_jj^-1 (b_j - sum_k L(j, k) y_k), k ascending
    for (int rd = 0; rd < c.nrounds; ++rd) {
        const int c0 = c.round_begin[rd];
        ex.each(c.round_begin[rd + 1] - c0, [&](int idx) {
            const int col = c0 + idx;
            double v[7];
ORBX_UNROLL
            for (int r = 0; r < 7; ++r) v[r] = c.bv[7 * col + r];
            for (int k = c.row_begin[col]; k < c.row_begin[col + 1]; ++k) {
                const int b = c.row_blk[k];
                const double *L = c.Lb + 49 * (size_t)b, *yk = c.y + 7 * c.blk_ij[2 * b + 1];
ORBX_UNROLL
                for (int r = 0; r < 7; ++r) v[r] = v[r] - orbx_eg_dot7(L + 7 * r, yk);
            }
            const double *Ljj = c.Lb + 49 * (size_t)c.blk_begin[col];
ORBX_UNROLL
            for (int r = 1; r < 7; ++r)
ORBX_UNROLL
                for (int m = 0; m < r; ++m) v[r] = v[r] - Ljj[7 * r + m] * v[m];
ORBX_UNROLL
            for (int r = 0; r < 7; ++r) c.y[7 * col + r] = v[r];
        });
    }
    // D L^T x = y: x_j = L_jj^-T (D_j^-1 y_j - sum_i L(i, j)^T x_i), i ascending
    for (int rd = c.nrounds - 1; rd >= 0; --rd) {
        const int c0 = c.round_begin[rd];
        ex.each(c.round_begin[rd + 1] - c0, [&](int idx) {
            const int col = c0 + idx;
            double v[7];
ORBX_UNROLL
            for (int cc = 0; cc < 7; ++cc) v[cc] = c.y[7 * col + cc] / c.dd[7 * col + cc];
            for (int b = c.blk_begin[col] + 1; b < c.blk_begin[col + 1]; ++b) {
                const double *L = c.Lb + 49 * (size_t)b, *xi = c.x + 7 * c.blk_ij[2 * b];
ORBX_UNROLL
                for (int cc = 0; cc < 7; ++cc) {
                    double s = L[cc] * xi[0];
ORBX_UNROLL
                    for (int r = 1; r < 7; ++r) s = s + L[7 * r + cc] * xi[r];
                    v[cc] = v[cc] - s;
                }
            }
            const double *Ljj = c.Lb + 49 * (size_t)c.blk_begin[col];
ORBX_UNROLL
            for (int cc = 5; cc >= 0; --cc)
ORBX_UNROLL
                for (int m = cc + 1; m < 7; ++m) v[cc] = v[cc] - Ljj[7 * m + cc] * v[m];
ORBX_UNROLL
            for (int cc = 0; cc < 7; ++cc) c.x[7 * col + cc] = v[cc];
        });
    }
    return true;
}
// push + update: every vertex is backed up, every active one takes its oplus (which zeroes x[6] in place under fix_scale)
template <class Ex> ORBX_HD static inline void orbx_eg_update(Ex &ex, const OrbxEgCtx &c) {
    ex.each(c.nv, [&](int v) {
        c.bak[v] = c.est[v];
        const int col = c.acol[v];
        if (col < 0) return;
        double u[7];
ORBX_UNROLL
        for (int j = 0; j < 7; ++j) u[j] = c.x[7 * col + j];
        c.est[v] = orbx_sim3opt_oplus(c.est[v], u, c.fix_scale != 0);
        c.x[7 * col + 6] = u[6];
    });
}
template <class Ex> ORBX_HD static inline void orbx_eg_restore(Ex &ex, const OrbxEgCtx &c) {
    ex.each(c.nv, [&](int v) { c.est[v] = c.bak[v]; });
}

// initializeOptimization() + optimize(20): orbx_localba_optimize's control with the user's lambda, no robust weight
template <class Ex> ORBX_HD static inline void orbx_eg_optimize(Ex &ex, const OrbxEgCtx &c, orbx_essgraph_result &R) {
    if (c.nact == 0) return;                                   // no active vertex: optimize() returns at once
    double lambda = 0.0, nu = 2.0, cur = 0.0;
    int stall = 0, it = 0, failed = 0;
    while (it < ORBX_EG_ITERS) {
        cur = orbx_eg_system(ex, c);
        const double ini = cur;
        if (it == 0) {
            R.chi2[0] = cur;
            lambda = ORBX_EG_LAMBDA0;                          // computeLambdaInit: _userLambdaInit > 0
            nu = 2.0;
            stall = 0;
        }
        ++it;
        double rho = 0.0;
        int q = 0;
        do {
            const bool ok = orbx_eg_solve(ex, c, lambda);
            if (!ok) ++failed;
            orbx_eg_update(ex, c);
            double tmp = orbx_eg_chi(ex, c);
            if (!ok) tmp = ORBX_DBL_MAX;
            rho = cur - tmp;
            const double scale = orbx_eg_scale(ex, c, lambda) + 1e-3;
            rho = rho / scale;
            if (rho > 0 && orbx_finite(tmp)) {
                const double r2 = 2.0 * rho - 1.0;
                double alpha = 1.0 - (r2 * r2) * r2;
                alpha = (2.0 / 3.0) < alpha ? (2.0 / 3.0) : alpha;
                const double sf = (1.0 / 3.0) < alpha ? alpha : (1.0 / 3.0);
                lambda = lambda * sf;
                nu = 2.0;
                cur = tmp;
            } else {
                lambda = lambda * nu;
                nu = nu * 2.0;
                orbx_eg_restore(ex, c);
            }
            ++q;
        } while (rho < 0 && q < ORBX_LM_TRIALS);
        if (q == ORBX_LM_TRIALS || rho == 0) break;            // Terminate
        if ((ini - cur) * 1e3 < ini) ++stall; else stall = 0;
        if (stall >= 3) break;                                  // Stop criterium (Raul)
    }
    R.iters = it; R.nfailed = failed;
    R.chi2[1] = cur; R.lambda = lambda;
}

template <class Ex> ORBX_HD static inline void orbx_eg_run(Ex &ex, const OrbxEgCtx &c, orbx_essgraph_result *res) {
    orbx_essgraph_result R;
    R.iters = 0; R.nactive = c.nact; R.nfailed = 0; R.nrounds = c.nrounds; R.nlblocks = c.nblk; R.pad = 0;
    R.chi2[0] = 0.0; R.chi2[1] = 0.0; R.lambda = 0.0;
    // vScw and the measurements (:1145-1163, :1185-1212): a loop connection takes both poses from vScw, the other edges prefer
    // NonCorrectedSim3
    ex.each(c.nv + c.ne, [&](int i) {
        if (i < c.nv) { c.est[i] = orbx_sim3opt_fetch(c.Scw + 8 * (size_t)i); c.bak[i] = c.est[i]; return; }
        const int e = i - c.nv;
        const double *src = c.edges[3 * e + 2] ? c.Scw : c.Snc;
        const OrbxSim3 Swi = orbx_sim3opt_inverse(orbx_sim3opt_fetch(src + 8 * (size_t)c.edges[3 * e]));
        orbx_sim3opt_store(orbx_sim3opt_mul(orbx_sim3opt_fetch(src + 8 * (size_t)c.edges[3 * e + 1]), Swi), c.meas + 8 * (size_t)e);
    });
    orbx_eg_optimize(ex, c, R);
    // :1304-1321: CorrectedSiw and Tiw = [R, t / s] narrowed to float
    ex.each(c.nv, [&](int v) {
        const OrbxSim3 S = c.est[v];
        double o[8], m[9];
        orbx_sim3opt_store(S, o);
ORBX_UNROLL
        for (int k = 0; k < 8; ++k) c.Siw_out[8 * (size_t)v + k] = orbx_canond(o[k]);
        orbx_pose_R_from_quat(S.q, m);
        const double is = 1.0 / S.s;
        float *T = c.Tiw_out + 16 * (size_t)v;
ORBX_UNROLL
        for (int r = 0; r < 3; ++r)
ORBX_UNROLL
            for (int cc = 0; cc < 3; ++cc) T[4 * r + cc] = orbx_canonf((float)m[3 * r + cc]);
        T[3] = orbx_canonf((float)(S.q.tx * is)); T[7] = orbx_canonf((float)(S.q.ty * is)); T[11] = orbx_canonf((float)(S.q.tz * is));
        T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
    });
    R.chi2[0] = orbx_canond(R.chi2[0]); R.chi2[1] = orbx_canond(R.chi2[1]); R.lambda = orbx_canond(R.lambda);
    if (ex.lead()) *res = R;
}

// Step 7 (:1326-1357), one point of the call: correctedSwr.map(Srw.map(P)) in double, rounded to float once; Srw = vScw[ref],
// correctedSwr = the inverse of the corrected Siw as the output block holds it.  ref < 0 (a bad point) is copied through.
ORBX_HD static inline void orbx_eg_correct_point(const DEgProb *prob, const uint8_t *in, const uint8_t *out, const float *world,
                                                 const int32_t *ref, const int32_t *pprob, float *world_out, int64_t i) {
    const int r = ref[i];
    if (r < 0) {
ORBX_UNROLL
        for (int a = 0; a < 3; ++a) world_out[3 * i + a] = world[3 * i + a];
        return;
    }
    const DEgProb &P = prob[pprob[i]];
    OrbxEgCtx c;
    orbx_eg_bind(P, in + P.o_in, nullptr, (uint8_t *)out + P.o_out, c);
    const OrbxSim3 Srw = orbx_sim3opt_fetch(c.Scw + 8 * (size_t)r);
    const OrbxSim3 Swr = orbx_sim3opt_inverse(orbx_sim3opt_fetch(c.Siw_out + 8 * (size_t)r));
    double p[3], q[3];
    orbx_pose_rotate(Srw.q, (double)world[3 * i], (double)world[3 * i + 1], (double)world[3 * i + 2], p);
    p[0] = Srw.s * p[0] + Srw.q.tx; p[1] = Srw.s * p[1] + Srw.q.ty; p[2] = Srw.s * p[2] + Srw.q.tz;
    orbx_pose_rotate(Swr.q, p[0], p[1], p[2], q);
    world_out[3 * i] = orbx_canonf((float)(Swr.s * q[0] + Swr.q.tx));
    world_out[3 * i + 1] = orbx_canonf((float)(Swr.s * q[1] + Swr.q.ty));
    world_out[3 * i + 2] = orbx_canonf((float)(Swr.s * q[2] + Swr.q.tz));
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side (orbx_essgraph.cpp, HIP-free: tools/san_essgraph.cpp builds it alone under the sanitizers).
// The symbolic part of one problem: the elimination order in rounds and the block structure of L with its index lists.
struct OrbxEgSymbolic {
    std::vector<int32_t> acol, col_vertex, inc_begin, inc, round_begin, blk_begin, blk_ij, pair_begin, pair, aent_begin, aent,
        row_begin, row_blk;
    bool over_cap = false;          // stopped counting above max_blocks
};
// max_blocks < 0: no cap.  edges: [ne][3]; fixed: [nv]
void orbx_eg_symbolic(int nv, int ne, const int32_t *edges, const uint8_t *fixed, long long max_blocks, OrbxEgSymbolic &sym);
struct OrbxEgPlan {
    int nproblems = 0;
    size_t o_prob = 0, in_bytes = 0, work_bytes = 0, out_bytes = 0;   // the input block starts with DEgProb[nproblems]
    size_t o_pts_in = 0, o_pts_out = 0;
    int64_t npoints = 0;
    std::vector<DEgProb> probs;
    std::vector<OrbxEgSymbolic> sym;
};
orbx_status orbx_eg_plan(int nproblems, const orbx_essgraph_problem *problems, const orbx_essgraph_result *results, bool cap,
                         OrbxEgPlan &plan, const char **why);
void orbx_eg_pack(const orbx_essgraph_problem *problems, const OrbxEgPlan &plan, uint8_t *dst);
void orbx_eg_host_run(const OrbxEgPlan &plan, const uint8_t *in, uint8_t *work, uint8_t *out);
void orbx_eg_unpack(const orbx_essgraph_problem *problems, const OrbxEgPlan &plan, const uint8_t *out, orbx_essgraph_result *results);
