// orbx_localba.h -- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:710-991) as scalar code shared by the host path
// (orbx_localba.cpp) and the kernel (k_local_ba): what g2o executes for VertexSE3Expmap keyframes and marginalised
// VertexSBAPointXYZ points joined by EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ edges -- buildSystem, the Schur complement over
// the free keyframes (BlockSolver_6_3::solve), Levenberg-Marquardt over all free vertices, and the two rounds with their
// classifications.  tests/localba_model.py restates it independently in numpy float64; DESIGN.md section 2 (F19) lists what was
// read from the reference and every arithmetic order this file fixes for itself where the reference leaves it to Eigen or to a
// sparse Cholesky.
//
// ONE ORDER PER SUM.  The work is cut into phases; a phase is a loop over independent items (points, edges, (keyframe, chain)
// pairs, rows of the reduced system) whose bodies read what earlier phases wrote and write disjoint places.  orbx_localba_run
// is written against an executor Ex with each(n, f) = "f(i) for every i in [0, n), then all of it is visible" -- a plain loop
// on the host, lanes striding over i and a barrier in the kernel -- so the host path and the device run the same bodies and
// every sum has the same order on both.  Long sums over a keyframe's edges and over the vertices take ORBX_LBA_CHAINS
// interleaved chains (chain c adds entries c, c + 64, ...), whose partials are then added in order of c.  The control values
// (chi2, lambda, rho, ...) come from such sums and are the same in every lane, so every branch around a barrier is uniform.
//
// fp_mode: every expression is written operation by operation and the library is built with -ffp-contract=off; the only fused
// operations are the explicit ones inside orbx_pose_sincos.  Both fp_modes give the same bits on the host and on the device.
#pragma once
#include <vector>
#include "orbx_pose.h"     // orbx_lm.h (Huber, orbx_finite, the term order), the SE3 pieces, orbx_pose_error
#include "orbx_ransac.h"   // orbx_canonf / orbx_canond, orbx_pad256

enum {
    ORBX_LBA_MAX_LOCAL = 128,       // local keyframes per problem: the reduced system is at most 768 x 768 doubles (4.5 MiB)
    ORBX_LBA_MAX_OBS = 4000000,     // observations per problem: 27 terms per edge stay inside 32-bit indices
    ORBX_LBA_MAX_ENT = 1 << 30,     // Schur pair entries per problem
    ORBX_LBA_CHAINS = 64,
    ORBX_LBA_KT = 27,               // per edge and keyframe: 21 of H_pp (upper triangle row by row), 6 of b_p
    ORBX_LBA_ITERS1 = 5, ORBX_LBA_ITERS2 = 10,
    ORBX_LBA_THREADS = 256
};
#define ORBX_LBA_CHI2_MONO 5.991
#define ORBX_LBA_CHI2_STEREO 7.815

// One problem as the kernel reads it: the counts and where its three blocks start (bytes from the call's input, workspace and
// output blocks).  Every array inside a block follows from the counts (orbx_localba_bind).
struct DLbaProb {
    int32_t nlocal, nfixed, npoints, nobs, nfree, nkfe, nent, second_round;
    float cam[4], bf;
    int32_t debug;                  // orbx_debug_localba_classify: the classification alone
    int64_t o_in, o_work, o_out;
};
static_assert(sizeof(DLbaProb) == 80, "packed for the device");
struct DLbaArgs {                   // k_local_ba: device pointers
    const DLbaProb *prob;
    const uint8_t *in;
    uint8_t *work, *out;
    int nproblems;                  // the results stand at the start of out
};

struct OrbxLbaCtx {
    int nlocal, nkf, npoints, nobs, nfree, nkfe, nblk, nent, second_round, debug;
    OrbxPoseCam K;
    // input block
    const float *Tcw;               // [nkf][16]
    const float *world;             // [npoints][3]
    const float *obs;               // [nobs][3]
    const float *w;                 // [nobs]
    const int32_t *obs_begin;       // [npoints + 1]
    const int32_t *obs_kf;          // [nobs]
    const int32_t *edge_pt;         // [nobs] the point of an edge
    const int32_t *fcol;            // [nkf] index among the free keyframes, -1: fixed
    const int32_t *free_kf;         // [nfree]
    const int32_t *kf_begin;        // [nfree + 1] edges by free keyframe,
    const int32_t *kf_edge;         // [nkfe]      ascending edge index
    const int32_t *blk_begin;       // [nblk + 1]  Schur blocks (i1 <= i2), i1-major; nblk = nfree (nfree + 1) / 2
    const int32_t *blk_ij;          // [nblk][2]
    const int32_t *blk_ent;         // [nent][2]   (edge on i1, edge on i2) of one point, points ascending
    const float *dbg;               // debug: Tcw_est [nkf][16] | world_est [npoints][3] | Tcw_last | world_last
    // workspace
    OrbxPoseSE3 *pose, *pose_bak;   // [nkf]
    double *pt, *pt_bak;            // [npoints][3]
    double *echi;                   // [nobs] chi2 of the edge where computeActiveErrors saw it last
    double *Hpl, *Y, *Ept;          // [nobs][18] H_pl (6 x 3), H_pl Dinv; [nobs][27]
    double *Hll, *bl, *Dinv, *Dbl, *cp, *xl;   // [npoints][6 | 3 | 6 | 3 | 1 | 3]
    double *Hpp;                    // [nfree][27]
    double *part;                   // [nfree][64][27]
    double *S, *d, *y, *x;          // [n][n], [n] each, n = 6 nfree
    double *red;                    // [64]
    int32_t *ccol;                  // [nfree] column block among the ACTIVE free keyframes, -1: no active edge
    int32_t *iw;                    // [4]: solve ok, active keyframes, any active edge
    uint8_t *flag, *pact;           // [nobs] level 1; [npoints] the point has an active edge
    // output block
    float *Tcw_out, *world_out;     // [nlocal][16], [npoints][3]
    uint8_t *erase;                 // [nobs]
};

struct OrbxLbaCarve {
    uint8_t *base; size_t off;
    template <class T> ORBX_HD T *take(size_t n) {
        off = (off + 7) & ~(size_t)7;
        T *p = (T *)(base + off);
        off += n * sizeof(T);
        return p;
    }
};
struct OrbxLbaSizes { size_t in_bytes, work_bytes, out_bytes; };
// The layout of a problem's three blocks.  With null bases only the sizes mean anything.
ORBX_HD static inline OrbxLbaSizes orbx_localba_bind(const DLbaProb &P, const uint8_t *in, uint8_t *work, uint8_t *out, OrbxLbaCtx &c) {
    c.nlocal = P.nlocal; c.nkf = P.nlocal + P.nfixed; c.npoints = P.npoints; c.nobs = P.nobs; c.nfree = P.nfree; c.nkfe = P.nkfe;
    c.nblk = P.nfree * (P.nfree + 1) / 2; c.nent = P.nent; c.second_round = P.second_round; c.debug = P.debug;
    c.K.fx = (double)P.cam[0]; c.K.fy = (double)P.cam[1]; c.K.cx = (double)P.cam[2]; c.K.cy = (double)P.cam[3]; c.K.bf = (double)P.bf;
    const size_t nkf = (size_t)c.nkf, np = (size_t)c.npoints, no = (size_t)c.nobs, nf = (size_t)c.nfree, n = 6 * nf;
    OrbxLbaSizes s;
    OrbxLbaCarve a = {(uint8_t *)in, 0};
    c.Tcw = a.take<float>(16 * nkf); c.world = a.take<float>(3 * np); c.obs = a.take<float>(3 * no); c.w = a.take<float>(no);
    c.obs_begin = a.take<int32_t>(np + 1); c.obs_kf = a.take<int32_t>(no); c.edge_pt = a.take<int32_t>(no);
    c.fcol = a.take<int32_t>(nkf); c.free_kf = a.take<int32_t>(nf); c.kf_begin = a.take<int32_t>(nf + 1);
    c.kf_edge = a.take<int32_t>((size_t)c.nkfe); c.blk_begin = a.take<int32_t>((size_t)c.nblk + 1);
    c.blk_ij = a.take<int32_t>(2 * (size_t)c.nblk); c.blk_ent = a.take<int32_t>(2 * (size_t)c.nent);
    c.dbg = a.take<float>(P.debug ? 2 * (16 * nkf + 3 * np) : 0);
    s.in_bytes = (a.off + 255) & ~(size_t)255;
    OrbxLbaCarve b = {work, 0};
    c.pose = b.take<OrbxPoseSE3>(nkf); c.pose_bak = b.take<OrbxPoseSE3>(nkf); c.pt = b.take<double>(3 * np); c.pt_bak = b.take<double>(3 * np);
    c.echi = b.take<double>(no); c.Hpl = b.take<double>(18 * no); c.Y = b.take<double>(18 * no); c.Ept = b.take<double>(ORBX_LBA_KT * no);
    c.Hll = b.take<double>(6 * np); c.bl = b.take<double>(3 * np); c.Dinv = b.take<double>(6 * np); c.Dbl = b.take<double>(3 * np);
    c.cp = b.take<double>(np); c.xl = b.take<double>(3 * np);
    c.Hpp = b.take<double>(ORBX_LBA_KT * nf); c.part = b.take<double>(ORBX_LBA_KT * ORBX_LBA_CHAINS * nf);
    c.S = b.take<double>(n * n); c.d = b.take<double>(n); c.y = b.take<double>(n); c.x = b.take<double>(n);
    c.red = b.take<double>(ORBX_LBA_CHAINS);
    c.ccol = b.take<int32_t>(nf); c.iw = b.take<int32_t>(4);
    c.flag = b.take<uint8_t>(no); c.pact = b.take<uint8_t>(np);
    s.work_bytes = (b.off + 255) & ~(size_t)255;
    OrbxLbaCarve o = {out, 0};
    c.Tcw_out = o.take<float>(16 * (size_t)c.nlocal); c.world_out = o.take<float>(3 * np); c.erase = o.take<uint8_t>(no);
    s.out_bytes = (o.off + 255) & ~(size_t)255;
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// One edge.
ORBX_HD static inline void orbx_localba_load(const OrbxLbaCtx &c, int e, const double *X, OrbxPoseEdge &E) {
    const float ur = c.obs[3 * e + 2];
    E.stereo = ur < 0 ? 0 : 1;                                  // mvuRight < 0: monocular edge
    E.ox = (double)c.obs[3 * e]; E.oy = (double)c.obs[3 * e + 1]; E.our = (double)ur;
    E.w = (double)c.w[e];
    E.X = X[0]; E.Y = X[1]; E.Z = X[2];
}
// computeError + chi2 at (T, X): orbx_pose_error, the edges' cam_project is the only-pose edges' (types_six_dof_expmap.cpp:141-158)
ORBX_HD static inline double orbx_localba_chi2(const OrbxLbaCtx &c, int e, const OrbxPoseSE3 *pose, const double *pt, int *stereo,
                                               double *pc, double *err, OrbxPoseEdge &E) {
    orbx_localba_load(c, e, pt + 3 * c.edge_pt[e], E);
    *stereo = E.stereo;
    return orbx_pose_error(pose[c.obs_kf[e]], c.K, E, pc, err);
}
// isDepthPositive: (T.map(X))(2) > 0.0 at the vertices' current estimates
ORBX_HD static inline bool orbx_localba_depth_positive(const OrbxLbaCtx &c, int e) {
    const OrbxPoseSE3 &T = c.pose[c.obs_kf[e]];
    const double *X = c.pt + 3 * c.edge_pt[e];
    double v[3];
    orbx_pose_rotate(T, X[0], X[1], X[2], v);
    return v[2] + T.tz > 0.0;
}
// linearizeOplus (types_six_dof_expmap.cpp:103-139, 188-234) at the camera-frame point pc: Ji [3][3] by the point, Jx [3][6] by
// the pose; row 2 is the stereo row.  Monocular Ji = (-1/z tmp) R with tmp's zeros left out of the products.
ORBX_HD static inline void orbx_localba_jac(const OrbxPoseSE3 &T, const OrbxPoseCam &K, int stereo, const double *pc, double *Ji, double *Jx) {
    double R[9];
    orbx_pose_R_from_quat(T, R);
    const double x = pc[0], y = pc[1], z = pc[2];
    const double z_2 = z * z;
    if (stereo) {
ORBX_UNROLL
        for (int a = 0; a < 3; ++a) {
            Ji[a] = (-K.fx * R[a]) / z + ((K.fx * x) * R[6 + a]) / z_2;
            Ji[3 + a] = (-K.fy * R[3 + a]) / z + ((K.fy * y) * R[6 + a]) / z_2;
            Ji[6 + a] = Ji[a] - (K.bf * R[6 + a]) / z_2;
        }
    } else {
        const double m = -1.0 / z;
        const double a00 = m * K.fx, a02 = m * ((-x / z) * K.fx), a11 = m * K.fy, a12 = m * ((-y / z) * K.fy);
ORBX_UNROLL
        for (int a = 0; a < 3; ++a) {
            Ji[a] = a00 * R[a] + a02 * R[6 + a];
            Ji[3 + a] = a11 * R[3 + a] + a12 * R[6 + a];
            Ji[6 + a] = 0.0;
        }
    }
    Jx[0] = ((x * y) / z_2) * K.fx;
    Jx[1] = -(1.0 + ((x * x) / z_2)) * K.fx;
    Jx[2] = (y / z) * K.fx;
    Jx[3] = (-1.0 / z) * K.fx;
    Jx[4] = 0.0;
    Jx[5] = (x / z_2) * K.fx;
    Jx[6] = (1.0 + (y * y) / z_2) * K.fy;
    Jx[7] = ((-x * y) / z_2) * K.fy;
    Jx[8] = (-x / z) * K.fy;
    Jx[9] = 0.0;
    Jx[10] = (-1.0 / z) * K.fy;
    Jx[11] = (y / z_2) * K.fy;
    if (stereo) {
        Jx[12] = Jx[0] - (K.bf * y) / z_2;
        Jx[13] = Jx[1] + (K.bf * x) / z_2;
        Jx[14] = Jx[2];
        Jx[15] = Jx[3];
        Jx[16] = 0.0;
        Jx[17] = Jx[5] - K.bf / z_2;
    } else {
ORBX_UNROLL
        for (int j = 12; j < 18; ++j) Jx[j] = 0.0;
    }
}
// sum over the edge's rows, r = 0, 1[, 2] in order
ORBX_HD static inline double orbx_localba_rows(int stereo, double r0, double r1, double r2) {
    const double s = r0 + r1;
    return stereo ? s + r2 : s;
}
// index of (j, k), j <= k, in the upper triangle of a 6 x 6 stored row by row
ORBX_HD static inline int orbx_localba_tri6(int j, int k) { return j * 6 - (j * (j - 1)) / 2 + (k - j); }

// computeActiveErrors + the point's share of activeRobustChi2 [+ buildSystem] over the active edges of point p, in CSR order
template <bool SYSTEM> ORBX_HD static inline void orbx_localba_point_pass(const OrbxLbaCtx &c, int p, bool robust) {
    double Hl[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bl[3] = {0.0, 0.0, 0.0}, cp = 0.0;
    if (c.pact[p]) {
        for (int e = c.obs_begin[p]; e < c.obs_begin[p + 1]; ++e) {
            if (c.flag[e]) continue;
            OrbxPoseEdge E;
            double pc[3], err[3], rho1;
            int stereo;
            const double chi2 = orbx_localba_chi2(c, e, c.pose, c.pt, &stereo, pc, err, E);
            c.echi[e] = chi2;
            cp = cp + orbx_pose_huber(chi2, stereo, robust, &rho1);
            if (!SYSTEM) continue;
            const int kf = c.obs_kf[e];
            double Ji[9], Jx[18];
            orbx_localba_jac(c.pose[kf], c.K, stereo, pc, Ji, Jx);
            const double W = rho1 * E.w;
            const double we0 = E.w * err[0], we1 = E.w * err[1], we2 = E.w * err[2];
            int n = 0;
ORBX_UNROLL
            for (int a = 0; a < 3; ++a)
ORBX_UNROLL
                for (int b = a; b < 3; ++b) {
                    Hl[n] = Hl[n] + orbx_localba_rows(stereo, (Ji[a] * W) * Ji[b], (Ji[3 + a] * W) * Ji[3 + b], (Ji[6 + a] * W) * Ji[6 + b]);
                    ++n;
                }
ORBX_UNROLL
            for (int a = 0; a < 3; ++a) bl[a] = bl[a] - rho1 * orbx_localba_rows(stereo, Ji[a] * we0, Ji[3 + a] * we1, Ji[6 + a] * we2);
            if (c.fcol[kf] < 0) continue;                      // a fixed keyframe: the point's H_ll / b_l only
            double *t = c.Ept + (size_t)ORBX_LBA_KT * e, *hpl = c.Hpl + (size_t)18 * e;
            n = 0;
ORBX_UNROLL
            for (int j = 0; j < 6; ++j)
ORBX_UNROLL
                for (int k = j; k < 6; ++k)
                    t[n++] = orbx_localba_rows(stereo, (Jx[j] * W) * Jx[k], (Jx[6 + j] * W) * Jx[6 + k], (Jx[12 + j] * W) * Jx[12 + k]);
ORBX_UNROLL
            for (int j = 0; j < 6; ++j) {
                t[21 + j] = rho1 * orbx_localba_rows(stereo, Jx[j] * we0, Jx[6 + j] * we1, Jx[12 + j] * we2);
ORBX_UNROLL
                for (int a = 0; a < 3; ++a)
                    hpl[3 * j + a] = orbx_localba_rows(stereo, (Jx[j] * W) * Ji[a], (Jx[6 + j] * W) * Ji[3 + a], (Jx[12 + j] * W) * Ji[6 + a]);
            }
        }
    }
    c.cp[p] = cp;
    if (SYSTEM) {
ORBX_UNROLL
        for (int k = 0; k < 6; ++k) c.Hll[6 * (size_t)p + k] = Hl[k];
ORBX_UNROLL
        for (int k = 0; k < 3; ++k) c.bl[3 * (size_t)p + k] = bl[k];
    }
}

// The partials in c.red added in order of the chain; every lane gets the same value
template <class Ex> ORBX_HD static inline double orbx_localba_sum64(Ex &ex, const OrbxLbaCtx &c) {
    double s = 0.0;
    for (int k = 0; k < ORBX_LBA_CHAINS; ++k) s = s + c.red[k];
    ex.sync();
    return s;
}
// activeRobustChi2 from the points' shares
template <class Ex> ORBX_HD static inline double orbx_localba_chi_total(Ex &ex, const OrbxLbaCtx &c) {
    ex.each(ORBX_LBA_CHAINS, [&](int ch) {
        double s = 0.0;
        for (int p = ch; p < c.npoints; p += ORBX_LBA_CHAINS) s = s + c.cp[p];
        c.red[ch] = s;
    });
    return orbx_localba_sum64(ex, c);
}
// computeActiveErrors + activeRobustChi2 + buildSystem at the current estimates.  Returns the chi2.
template <class Ex> ORBX_HD static inline double orbx_localba_system(Ex &ex, const OrbxLbaCtx &c, bool robust) {
    ex.each(c.npoints, [&](int p) { orbx_localba_point_pass<true>(c, p, robust); });
    ex.each(c.nfree * ORBX_LBA_CHAINS, [&](int idx) {
        const int f = idx / ORBX_LBA_CHAINS, ch = idx % ORBX_LBA_CHAINS;
        double a[ORBX_LBA_KT];
ORBX_UNROLL
        for (int t = 0; t < ORBX_LBA_KT; ++t) a[t] = 0.0;
        for (int k = c.kf_begin[f] + ch; k < c.kf_begin[f + 1]; k += ORBX_LBA_CHAINS) {
            const int e = c.kf_edge[k];
            if (c.flag[e]) continue;
            const double *t = c.Ept + (size_t)ORBX_LBA_KT * e;
ORBX_UNROLL
            for (int j = 0; j < ORBX_LBA_KT; ++j) a[j] = orbx_lm_accumulate<6>(j, a[j], t[j]);
        }
ORBX_UNROLL
        for (int t = 0; t < ORBX_LBA_KT; ++t) c.part[(size_t)ORBX_LBA_KT * idx + t] = a[t];
    });
    ex.each(c.nfree * ORBX_LBA_KT, [&](int idx) {
        const int f = idx / ORBX_LBA_KT, t = idx % ORBX_LBA_KT;
        double s = 0.0;
        for (int ch = 0; ch < ORBX_LBA_CHAINS; ++ch) s = s + c.part[(size_t)ORBX_LBA_KT * (f * ORBX_LBA_CHAINS + ch) + t];
        c.Hpp[idx] = s;
    });
    return orbx_localba_chi_total(ex, c);
}
// computeActiveErrors + activeRobustChi2 at the current estimates
template <class Ex> ORBX_HD static inline double orbx_localba_chi(Ex &ex, const OrbxLbaCtx &c, bool robust) {
    ex.each(c.npoints, [&](int p) { orbx_localba_point_pass<false>(c, p, robust); });
    return orbx_localba_chi_total(ex, c);
}
// computeLambdaInit's max |H_jj| over the active keyframes and points: std::max as written, chains over the vertices
template <class Ex> ORBX_HD static inline double orbx_localba_max_diag(Ex &ex, const OrbxLbaCtx &c) {
    ex.each(ORBX_LBA_CHAINS, [&](int ch) {
        double m = 0.0;
        for (int f = ch; f < c.nfree; f += ORBX_LBA_CHAINS) {
            if (c.ccol[f] < 0) continue;
            int dg = 0;
            for (int j = 0; j < 6; ++j) { const double a = __builtin_fabs(c.Hpp[ORBX_LBA_KT * f + dg]); m = a < m ? m : a; dg += 6 - j; }
        }
        for (int p = ch; p < c.npoints; p += ORBX_LBA_CHAINS) {
            if (!c.pact[p]) continue;
            int dg = 0;
            for (int j = 0; j < 3; ++j) { const double a = __builtin_fabs(c.Hll[6 * (size_t)p + dg]); m = a < m ? m : a; dg += 3 - j; }
        }
        c.red[ch] = m;
    });
    double m = 0.0;
    for (int k = 0; k < ORBX_LBA_CHAINS; ++k) { const double a = c.red[k]; m = a < m ? m : a; }
    ex.sync();
    return m;
}
// computeScale over the whole x: sum x_j (lambda x_j + b_j), chains over the vertices
template <class Ex> ORBX_HD static inline double orbx_localba_scale(Ex &ex, const OrbxLbaCtx &c, double lambda) {
    ex.each(ORBX_LBA_CHAINS, [&](int ch) {
        double s = 0.0;
        for (int f = ch; f < c.nfree; f += ORBX_LBA_CHAINS) {
            const int cc = c.ccol[f];
            if (cc < 0) continue;
            for (int j = 0; j < 6; ++j) { const double xv = c.x[6 * cc + j]; s = s + xv * (lambda * xv + c.Hpp[ORBX_LBA_KT * f + 21 + j]); }
        }
        for (int p = ch; p < c.npoints; p += ORBX_LBA_CHAINS) {
            if (!c.pact[p]) continue;
            for (int j = 0; j < 3; ++j) { const double xv = c.xl[3 * (size_t)p + j]; s = s + xv * (lambda * xv + c.bl[3 * (size_t)p + j]); }
        }
        c.red[ch] = s;
    });
    return orbx_localba_sum64(ex, c);
}

// BlockSolver::solve with lambda on every diagonal: Dinv, the Schur complement, the dense unpivoted L D L^T (fails when a pivot is
// not positive and finite: then x = 0, as orbx_lm_solve), x_p, x_l.  n = 6 x active keyframes.
template <class Ex> ORBX_HD static inline bool orbx_localba_solve(Ex &ex, const OrbxLbaCtx &c, int n, double lambda) {
    ex.each(c.npoints, [&](int p) {
        if (!c.pact[p]) return;
        const double *h = c.Hll + 6 * (size_t)p, *b = c.bl + 3 * (size_t)p;
        const double a00 = h[0] + lambda, a01 = h[1], a02 = h[2], a11 = h[3] + lambda, a12 = h[4], a22 = h[5] + lambda;
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double det = (a00 * c00 + a01 * c01) + a02 * c02;
        const double id = 1.0 / det;
        double *D = c.Dinv + 6 * (size_t)p, *db = c.Dbl + 3 * (size_t)p;
        D[0] = c00 * id; D[1] = c01 * id; D[2] = c02 * id; D[3] = c11 * id; D[4] = c12 * id; D[5] = c22 * id;
        db[0] = (D[0] * b[0] + D[1] * b[1]) + D[2] * b[2];
        db[1] = (D[1] * b[0] + D[3] * b[1]) + D[4] * b[2];
        db[2] = (D[2] * b[0] + D[4] * b[1]) + D[5] * b[2];
    });
    ex.each(c.nobs, [&](int e) {
        if (c.flag[e] || c.fcol[c.obs_kf[e]] < 0) return;
        const double *D = c.Dinv + 6 * (size_t)c.edge_pt[e], *h = c.Hpl + 18 * (size_t)e;
        double *yv = c.Y + 18 * (size_t)e;
ORBX_UNROLL
        for (int j = 0; j < 6; ++j) {
            yv[3 * j] = (h[3 * j] * D[0] + h[3 * j + 1] * D[1]) + h[3 * j + 2] * D[2];
            yv[3 * j + 1] = (h[3 * j] * D[1] + h[3 * j + 1] * D[3]) + h[3 * j + 2] * D[4];
            yv[3 * j + 2] = (h[3 * j] * D[2] + h[3 * j + 1] * D[4]) + h[3 * j + 2] * D[5];
        }
    });
    // S = H_pp + lambda I - sum_l H_pl Dinv H_pl^T, block (i1, i2) row r per item; the lower triangle is what the solve reads
    ex.each(c.nblk * 6, [&](int idx) {
        const int b = idx / 6, r = idx % 6;
        const int i1 = c.blk_ij[2 * b], i2 = c.blk_ij[2 * b + 1];
        const int c1 = c.ccol[i1], c2 = c.ccol[i2];
        if (c1 < 0 || c2 < 0) return;
        double acc[6];
ORBX_UNROLL
        for (int k = 0; k < 6; ++k) {
            acc[k] = 0.0;
            if (i1 == i2) {
                const double v = c.Hpp[ORBX_LBA_KT * i1 + (r <= k ? orbx_localba_tri6(r, k) : orbx_localba_tri6(k, r))];
                acc[k] = r == k ? v + lambda : v;
            }
        }
        for (int k = c.blk_begin[b]; k < c.blk_begin[b + 1]; ++k) {
            const int ea = c.blk_ent[2 * k], eb = c.blk_ent[2 * k + 1];
            if (c.flag[ea] || c.flag[eb]) continue;
            const double *ya = c.Y + 18 * (size_t)ea + 3 * r, *hb = c.Hpl + 18 * (size_t)eb;
ORBX_UNROLL
            for (int k2 = 0; k2 < 6; ++k2) acc[k2] = acc[k2] - ((ya[0] * hb[3 * k2] + ya[1] * hb[3 * k2 + 1]) + ya[2] * hb[3 * k2 + 2]);
        }
ORBX_UNROLL
        for (int k = 0; k < 6; ++k)
            if (i1 < i2 || k >= r) c.S[(size_t)(6 * c2 + k) * n + 6 * c1 + r] = acc[k];
    });
    // b_s = b_p - sum_l H_pl Dinv b_l, the keyframe's edges in 64 chains
    ex.each(c.nfree * ORBX_LBA_CHAINS, [&](int idx) {
        const int f = idx / ORBX_LBA_CHAINS, ch = idx % ORBX_LBA_CHAINS;
        double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = c.kf_begin[f] + ch; k < c.kf_begin[f + 1]; k += ORBX_LBA_CHAINS) {
            const int e = c.kf_edge[k];
            if (c.flag[e]) continue;
            const double *h = c.Hpl + 18 * (size_t)e, *db = c.Dbl + 3 * (size_t)c.edge_pt[e];
ORBX_UNROLL
            for (int r = 0; r < 6; ++r) a[r] = a[r] + ((h[3 * r] * db[0] + h[3 * r + 1] * db[1]) + h[3 * r + 2] * db[2]);
        }
ORBX_UNROLL
        for (int r = 0; r < 6; ++r) c.part[(size_t)ORBX_LBA_KT * idx + r] = a[r];
    });
    ex.each(c.nfree * 6, [&](int idx) {
        const int f = idx / 6, r = idx % 6;
        const int cc = c.ccol[f];
        if (cc < 0) return;
        double s = 0.0;
        for (int ch = 0; ch < ORBX_LBA_CHAINS; ++ch) s = s + c.part[(size_t)ORBX_LBA_KT * (f * ORBX_LBA_CHAINS + ch) + r];
        c.y[6 * cc + r] = c.Hpp[ORBX_LBA_KT * f + 21 + r] - s;
    });
    // L D L^T, left-looking: in column j every row i >= j is one chain over k < j, k ascending (row j's chain is the pivot and
    // every item of the column runs it for itself); L overwrites the strict lower triangle
    for (int j = 0; j < n; ++j)
        ex.each(n - j, [&](int idx) {
            const int i = j + idx;
            const double *rj = c.S + (size_t)j * n;
            double *ri = c.S + (size_t)i * n;
            double s = rj[j], t = ri[j];
            for (int k = 0; k < j; ++k) {
                const double wv = rj[k] * c.d[k];
                s = s - rj[k] * wv;
                t = t - ri[k] * wv;
            }
            if (i == j) c.d[j] = s; else ri[j] = t / s;
        });
    ex.each(1, [&](int) { c.iw[0] = 1; });
    ex.each(n, [&](int i) { if (!(c.d[i] > 0 && c.d[i] <= ORBX_DBL_MAX)) c.iw[0] = 0; });
    const bool ok = c.iw[0] != 0;
    ex.sync();
    if (ok) {
        // L y = b_s: once y_k stands, every row below takes its term -- per row the terms come in order of k ascending
        for (int k = 0; k + 1 < n; ++k)
            ex.each(n - k - 1, [&](int idx) { const int i = k + 1 + idx; c.y[i] = c.y[i] - c.S[(size_t)i * n + k] * c.y[k]; });
        // D L^T x = y: x_i = y_i / d_i, then once x_k stands every row above takes its term -- per row k descending
        ex.each(n, [&](int i) { c.x[i] = c.y[i] / c.d[i]; });
        for (int k = n - 1; k > 0; --k)
            ex.each(k, [&](int i) { c.x[i] = c.x[i] - c.S[(size_t)k * n + i] * c.x[k]; });
    } else {
        ex.each(n, [&](int i) { c.x[i] = 0.0; });
    }
    // x_l = Dinv (b_l - H_pl^T x_p), the point's edges in CSR order
    ex.each(c.npoints, [&](int p) {
        if (!c.pact[p]) return;
        double *xl = c.xl + 3 * (size_t)p;
        if (!ok) { xl[0] = 0.0; xl[1] = 0.0; xl[2] = 0.0; return; }
        double v[3] = {c.bl[3 * (size_t)p], c.bl[3 * (size_t)p + 1], c.bl[3 * (size_t)p + 2]};
        for (int e = c.obs_begin[p]; e < c.obs_begin[p + 1]; ++e) {
            const int f = c.fcol[c.obs_kf[e]];
            if (c.flag[e] || f < 0) continue;
            const double *h = c.Hpl + 18 * (size_t)e, *xp = c.x + 6 * c.ccol[f];
ORBX_UNROLL
            for (int a = 0; a < 3; ++a) {
                double s = h[a] * xp[0];
ORBX_UNROLL
                for (int j = 1; j < 6; ++j) s = s + h[3 * j + a] * xp[j];
                v[a] = v[a] - s;
            }
        }
        const double *D = c.Dinv + 6 * (size_t)p;
        xl[0] = (D[0] * v[0] + D[1] * v[1]) + D[2] * v[2];
        xl[1] = (D[1] * v[0] + D[3] * v[1]) + D[4] * v[2];
        xl[2] = (D[2] * v[0] + D[4] * v[1]) + D[5] * v[2];
    });
    return ok;
}
// push + update: every free vertex is backed up, every active one takes its oplus (exp(x) * T; X + x)
template <class Ex> ORBX_HD static inline void orbx_localba_update(Ex &ex, const OrbxLbaCtx &c) {
    ex.each(c.nfree + c.npoints, [&](int i) {
        if (i < c.nfree) {
            const int kf = c.free_kf[i], cc = c.ccol[i];
            c.pose_bak[kf] = c.pose[kf];
            if (cc < 0) return;
            double u[6];
ORBX_UNROLL
            for (int j = 0; j < 6; ++j) u[j] = c.x[6 * cc + j];
            c.pose[kf] = orbx_pose_mul(orbx_pose_exp(u), c.pose[kf]);
        } else {
            const size_t p = (size_t)(i - c.nfree);
ORBX_UNROLL
            for (int a = 0; a < 3; ++a) {
                c.pt_bak[3 * p + a] = c.pt[3 * p + a];
                if (c.pact[p]) c.pt[3 * p + a] = c.pt[3 * p + a] + c.xl[3 * p + a];
            }
        }
    });
}
// pop
template <class Ex> ORBX_HD static inline void orbx_localba_restore(Ex &ex, const OrbxLbaCtx &c) {
    ex.each(c.nfree + c.npoints, [&](int i) {
        if (i < c.nfree) { const int kf = c.free_kf[i]; c.pose[kf] = c.pose_bak[kf]; }
        else { const size_t p = (size_t)(i - c.nfree); c.pt[3 * p] = c.pt_bak[3 * p]; c.pt[3 * p + 1] = c.pt_bak[3 * p + 1]; c.pt[3 * p + 2] = c.pt_bak[3 * p + 2]; }
    });
}

// initializeOptimization(0) + optimize(iters): the active sets, then the control of orbx_lm_optimize over all free vertices.
// Returns the iterations run; chi2[0] = activeRobustChi2 at the first linearisation, chi2[1] = the last accepted one.
template <class Ex> ORBX_HD static inline int orbx_localba_optimize(Ex &ex, const OrbxLbaCtx &c, int iters, bool robust, double *chi2) {
    ex.each(c.npoints + c.nfree, [&](int i) {
        if (i < c.npoints) {
            uint8_t any = 0;
            for (int e = c.obs_begin[i]; e < c.obs_begin[i + 1]; ++e) if (!c.flag[e]) any = 1;
            c.pact[i] = any;
        } else {
            const int f = i - c.npoints;
            int any = -1;
            for (int k = c.kf_begin[f]; k < c.kf_begin[f + 1]; ++k) if (!c.flag[c.kf_edge[k]]) any = 0;
            c.ccol[f] = any;
        }
    });
    ex.each(1, [&](int) {
        int na = 0, anyp = 0;
        for (int f = 0; f < c.nfree; ++f) if (c.ccol[f] >= 0) c.ccol[f] = na++;
        for (int p = 0; p < c.npoints; ++p) if (c.pact[p]) anyp = 1;
        c.iw[1] = na; c.iw[2] = anyp;
    });
    const int n = 6 * c.iw[1];
    const bool any = c.iw[2] != 0;
    ex.sync();
    chi2[0] = 0.0; chi2[1] = 0.0;
    if (!any) return 0;                                        // no active edge: no active vertex, optimize() returns at once
    double lambda = 0.0, nu = 2.0, cur = 0.0;
    int stall = 0, it = 0;
    while (it < iters) {
        cur = orbx_localba_system(ex, c, robust);
        const double ini = cur;
        if (it == 0) {
            chi2[0] = cur;
            lambda = 1e-5 * orbx_localba_max_diag(ex, c);
            nu = 2.0;
            stall = 0;
        }
        ++it;
        double rho = 0.0;
        int q = 0;
        do {
            const bool ok = orbx_localba_solve(ex, c, n, lambda);
            orbx_localba_update(ex, c);
            double tmp = orbx_localba_chi(ex, c, robust);
            if (!ok) tmp = ORBX_DBL_MAX;
            rho = cur - tmp;
            const double scale = orbx_localba_scale(ex, c, lambda) + 1e-3;
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
                orbx_localba_restore(ex, c);
            }
            ++q;
        } while (rho < 0 && q < ORBX_LM_TRIALS);
        if (q == ORBX_LM_TRIALS || rho == 0) break;            // Terminate
        if ((ini - cur) * 1e3 < ini) ++stall; else stall = 0;
        if (stall >= 3) break;                                  // Stop criterium (Raul)
    }
    chi2[1] = cur;
    return it;
}
// The classification (src/Optimizer.cc:909-944, 958-991): chi2 as computeActiveErrors left it, the depth at the current estimates
ORBX_HD static inline bool orbx_localba_is_outlier(const OrbxLbaCtx &c, int e) {
    const double th = c.obs[3 * e + 2] < 0 ? ORBX_LBA_CHI2_MONO : ORBX_LBA_CHI2_STEREO;
    return c.echi[e] > th || !orbx_localba_depth_positive(c, e);
}

template <class Ex> ORBX_HD static inline void orbx_localba_run(Ex &ex, const OrbxLbaCtx &c, orbx_localba_result *res) {
    orbx_localba_result R;
    R.iters[0] = 0; R.iters[1] = 0; R.nflagged = 0; R.nerase = 0;
    R.chi2[0] = 0.0; R.chi2[1] = 0.0; R.chi2[2] = 0.0; R.chi2[3] = 0.0;
    const size_t dl = 16 * (size_t)c.nkf + 3 * (size_t)c.npoints;   // debug: where the "last" estimates start
    ex.each(c.nkf + c.npoints + c.nobs, [&](int i) {
        if (i < c.nkf) {
            c.pose[i] = orbx_pose_from_tcw((c.debug ? c.dbg : c.Tcw) + 16 * (size_t)i);
            c.pose_bak[i] = c.debug ? orbx_pose_from_tcw(c.dbg + dl + 16 * (size_t)i) : c.pose[i];
        } else if (i < c.nkf + c.npoints) {
            const size_t p = (size_t)(i - c.nkf);
            const float *src = c.debug ? c.dbg + 16 * (size_t)c.nkf : c.world;
ORBX_UNROLL
            for (int a = 0; a < 3; ++a) {
                c.pt[3 * p + a] = (double)src[3 * p + a];
                c.pt_bak[3 * p + a] = c.debug ? (double)c.dbg[dl + 16 * (size_t)c.nkf + 3 * p + a] : c.pt[3 * p + a];
            }
        } else {
            const int e = i - c.nkf - c.npoints;
            c.flag[e] = 0; c.echi[e] = 0.0;
        }
    });
    if (c.debug) {                                             // chi2 at the "last" estimates, the depth at the estimates
        ex.each(c.nobs, [&](int e) {
            OrbxPoseEdge E;
            double pc[3], err[3];
            int stereo;
            c.echi[e] = orbx_localba_chi2(c, e, c.pose_bak, c.pt_bak, &stereo, pc, err, E);
        });
    } else {
        R.iters[0] = orbx_localba_optimize(ex, c, ORBX_LBA_ITERS1, true, R.chi2);
        if (c.second_round) {
            ex.each(c.nobs, [&](int e) { c.flag[e] = orbx_localba_is_outlier(c, e) ? 1 : 0; });
            R.iters[1] = orbx_localba_optimize(ex, c, ORBX_LBA_ITERS2, false, R.chi2 + 2);
        }
    }
    ex.each(c.nobs + c.nlocal + c.npoints, [&](int i) {
        if (i < c.nobs) {
            c.erase[i] = orbx_localba_is_outlier(c, i) ? 1 : 0;
        } else if (c.debug) {
        } else if (i < c.nobs + c.nlocal) {
            const int k = i - c.nobs;
            float M[16];
            orbx_pose_to_tcw(c.pose[k], M);
ORBX_UNROLL
            for (int j = 0; j < 16; ++j) c.Tcw_out[16 * (size_t)k + j] = orbx_canonf(M[j]);
        } else {
            const size_t p = (size_t)(i - c.nobs - c.nlocal);
ORBX_UNROLL
            for (int a = 0; a < 3; ++a) c.world_out[3 * p + a] = orbx_canonf((float)c.pt[3 * p + a]);
        }
    });
    ex.each(ORBX_LBA_CHAINS, [&](int ch) {
        int ne = 0;
        for (int e = ch; e < c.nobs; e += ORBX_LBA_CHAINS) ne += c.erase[e];
        c.red[ch] = (double)ne;
    });
    R.nerase = (int)orbx_localba_sum64(ex, c);
    ex.each(ORBX_LBA_CHAINS, [&](int ch) {
        int nf = 0;
        for (int e = ch; e < c.nobs; e += ORBX_LBA_CHAINS) nf += c.flag[e];
        c.red[ch] = (double)nf;
    });
    R.nflagged = (int)orbx_localba_sum64(ex, c);
    for (int k = 0; k < 4; ++k) R.chi2[k] = orbx_canond(R.chi2[k]);
    if (ex.lead()) *res = R;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side (orbx_localba.cpp, HIP-free: tools/san_localba.cpp builds it alone under the sanitizers).
struct OrbxLbaPlan {
    int nproblems = 0;
    size_t o_prob = 0, in_bytes = 0, work_bytes = 0, out_bytes = 0;   // the input block starts with DLbaProb[nproblems]
};
orbx_status orbx_localba_plan(int nproblems, const orbx_localba_problem *problems, const orbx_localba_result *results,
                              const orbx_localba_debug *dbg, bool debug, OrbxLbaPlan &plan, std::vector<DLbaProb> &probs, const char **why);
void orbx_localba_pack(const orbx_localba_problem *problems, const orbx_localba_debug *dbg, const OrbxLbaPlan &plan,
                       const std::vector<DLbaProb> &probs, uint8_t *dst);
void orbx_localba_host_run(const OrbxLbaPlan &plan, const uint8_t *in, uint8_t *work, uint8_t *out);
void orbx_localba_unpack(const orbx_localba_problem *problems, const std::vector<DLbaProb> &probs, const uint8_t *out, bool debug,
                         orbx_localba_result *results);
