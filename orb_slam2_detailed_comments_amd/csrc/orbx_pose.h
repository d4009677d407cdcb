// orbx_pose.h -- Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:363-607) as scalar code shared by the host path
// (orbx_pose.cpp) and the kernel (k_pose_opt): what g2o executes for ONE VertexSE3Expmap with unary
// EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose edges, a dense 6x6 system and Levenberg-Marquardt.
// tests/pose_model.py restates it independently in numpy float64; DESIGN.md section 2 (F11) lists what was read from the
// reference and every arithmetic order this file fixes for itself where the reference leaves it to Eigen or libm.
//
// fp_mode: every expression below is written operation by operation and the library is built with -ffp-contract=off, so no
// multiply-add is contracted anywhere except inside orbx_pose_sincos, whose fused operations are explicit.  ORBX_FP_GCC_FMA
// and ORBX_FP_STRICT handles therefore give the same bits, on the host and on the device.  Division and square root are the
// correctly rounded IEEE double operations on both sides.  No pow, sin or cos of any math library is called.
#pragma once
#include "orbx_lm.h"   // ORBX_HD, ORBX_UNROLL, the Huber kernel, the 6 x 6 solve and the Levenberg-Marquardt loop

enum { ORBX_POSE_ROUNDS = 4, ORBX_POSE_ITERS = 10, ORBX_POSE_TERMS = OrbxLm<6>::TERMS };   // 21 of H, 6 of b, rho0
// (float)sqrt(5.991), (float)sqrt(7.815) widened: RobustKernelHuber::setDelta(deltaMono / deltaStereo), src/Optimizer.cc:407-409
#define ORBX_POSE_DELTA_MONO 0x1.394ca8p+1
#define ORBX_POSE_DELTA_STEREO 0x1.65d4p+1

struct OrbxPoseSE3 { double qx, qy, qz, qw, tx, ty, tz; };   // g2o::SE3Quat: _r (x, y, z, w), _t
struct OrbxPoseCam { double fx, fy, cx, cy, bf; };
struct OrbxPoseEdge { double ox, oy, our, w, X, Y, Z; int stereo; };   // obs, invSigma2, Xw: floats widened
// One problem as the edge loader sees it: the frame's rows and the problem's list.  Host pointers on the host path, device
// pointers in the kernel.
struct OrbxPoseView {
    const orbx_keypoint *kp;    // mvKeysUn of the frame
    const float *ur;            // mvuRight of the frame, or NULL (all mono)
    const int32_t *pt;          // the problem's d_point row
    const int32_t *index;       // list position -> pool index, or NULL
    const float *world;         // pool, 3 per point
    const float *sig;           // mvInvLevelSigma2
    int nlevels, npoints, n;    // n = min(count of the frame, cap)
};

// sin and cos of theta >= 0 for SE3Quat::exp.  Only *, +, fma and int conversion: pi/2 reduction in three parts, then the
// fdlibm kernel polynomials on [-pi/4, pi/4].  theta >= 2^30 or NaN (no tracking update) is defined as sin = 0, cos = 1.
ORBX_HD static inline void orbx_pose_sincos(double th, double *s, double *c) {
    if (!(th < 1073741824.0)) { *s = 0.0; *c = 1.0; return; }
    const double q = th * 0x1.45f306dc9c883p-1;
    const int n = (int)(q + 0.5);
    const double dn = -(double)n;
    double r = __builtin_fma(dn, 0x1.921fb54442d18p+0, th);
    r = __builtin_fma(dn, 0x1.1a62633145c07p-54, r);
    r = __builtin_fma(dn, -0x1.f1976b7ed8fbcp-110, r);
    const double z = r * r;
    double p = __builtin_fma(z, 0x1.5d93a5acfd57cp-33, -0x1.ae5e68a2b9cebp-26);
    p = __builtin_fma(z, p, 0x1.71de357b1fe7dp-19);
    p = __builtin_fma(z, p, -0x1.a01a019c161d5p-13);
    p = __builtin_fma(z, p, 0x1.111111110f8a6p-7);
    p = __builtin_fma(z, p, -0x1.5555555555549p-3);
    const double sn = __builtin_fma(z * r, p, r);
    double g = __builtin_fma(z, -0x1.8fae9be8838d4p-37, 0x1.1ee9ebdb4b1c4p-29);
    g = __builtin_fma(z, g, -0x1.27e4f809c52adp-22);
    g = __builtin_fma(z, g, 0x1.a01a019cb1590p-16);
    g = __builtin_fma(z, g, -0x1.6c16c16c15177p-10);
    g = __builtin_fma(z, g, 0x1.555555555554cp-5);
    const double cs = __builtin_fma(z * z, g, 1.0 - 0.5 * z);
    switch (n & 3) {
    case 0: *s = sn; *c = cs; break;
    case 1: *s = cs; *c = -sn; break;
    case 2: *s = -sn; *c = -cs; break;
    default: *s = -cs; *c = sn; break;
    }
}

// SE3Quat::normalizeRotation: w < 0 flips the sign, then every coefficient is divided by the norm (sum x, y, z, w in order)
ORBX_HD static inline void orbx_pose_normalize(OrbxPoseSE3 &T) {
    if (T.qw < 0) { T.qx = T.qx * -1.0; T.qy = T.qy * -1.0; T.qz = T.qz * -1.0; T.qw = T.qw * -1.0; }
    const double n = sqrt(T.qx * T.qx + T.qy * T.qy + T.qz * T.qz + T.qw * T.qw);
    T.qx = T.qx / n; T.qy = T.qy / n; T.qz = T.qz / n; T.qw = T.qw / n;
}
// Eigen::Quaterniond(Matrix3d) (QuaternionBase::operator=(MatrixBase), the trace > 0 branch and the three others); m row major
ORBX_HD static inline void orbx_pose_quat_from_R(const double *m, OrbxPoseSE3 &T) {
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        T.qw = 0.5 * t;
        t = 0.5 / t;
        T.qx = (m[7] - m[5]) * t; T.qy = (m[2] - m[6]) * t; T.qz = (m[3] - m[1]) * t;
    } else if (m[0] >= m[4] && m[0] >= m[8]) {          // i = 0, j = 1, k = 2
        t = sqrt(m[0] - m[4] - m[8] + 1.0);
        T.qx = 0.5 * t; t = 0.5 / t;
        T.qw = (m[7] - m[5]) * t; T.qy = (m[3] + m[1]) * t; T.qz = (m[6] + m[2]) * t;
    } else if (m[4] > m[0] && m[4] >= m[8]) {           // i = 1, j = 2, k = 0
        t = sqrt(m[4] - m[8] - m[0] + 1.0);
        T.qy = 0.5 * t; t = 0.5 / t;
        T.qw = (m[2] - m[6]) * t; T.qz = (m[7] + m[5]) * t; T.qx = (m[1] + m[3]) * t;
    } else {                                             // i = 2, j = 0, k = 1
        t = sqrt(m[8] - m[0] - m[4] + 1.0);
        T.qz = 0.5 * t; t = 0.5 / t;
        T.qw = (m[3] - m[1]) * t; T.qx = (m[2] + m[6]) * t; T.qy = (m[5] + m[7]) * t;
    }
}
// Quaterniond::toRotationMatrix, row major
ORBX_HD static inline void orbx_pose_R_from_quat(const OrbxPoseSE3 &T, double *m) {
    const double tx = 2.0 * T.qx, ty = 2.0 * T.qy, tz = 2.0 * T.qz;
    const double twx = tx * T.qw, twy = ty * T.qw, twz = tz * T.qw;
    const double txx = tx * T.qx, txy = ty * T.qx, txz = tz * T.qx;
    const double tyy = ty * T.qy, tyz = tz * T.qy, tzz = tz * T.qz;
    m[0] = 1.0 - (tyy + tzz); m[1] = txy - twz; m[2] = txz + twy;
    m[3] = txy + twz; m[4] = 1.0 - (txx + tzz); m[5] = tyz - twx;
    m[6] = txz - twy; m[7] = tyz + twx; m[8] = 1.0 - (txx + tyy);
}
// Quaterniond * Vector3d (_transformVector): uv = 2 (q.vec x v); v + w uv + q.vec x uv
ORBX_HD static inline void orbx_pose_rotate(const OrbxPoseSE3 &T, double vx, double vy, double vz, double *o) {
    double ux = T.qy * vz - T.qz * vy, uy = T.qz * vx - T.qx * vz, uz = T.qx * vy - T.qy * vx;
    ux = ux + ux; uy = uy + uy; uz = uz + uz;
    o[0] = (vx + T.qw * ux) + (T.qy * uz - T.qz * uy);
    o[1] = (vy + T.qw * uy) + (T.qz * ux - T.qx * uz);
    o[2] = (vz + T.qw * uz) + (T.qx * uy - T.qy * ux);
}
// Converter::toSE3Quat(cv::Mat): floats widened, SE3Quat(R, t)
ORBX_HD static inline OrbxPoseSE3 orbx_pose_from_tcw(const float *M) {
    double m[9];
    OrbxPoseSE3 T;
ORBX_UNROLL
    for (int r = 0; r < 3; ++r)
ORBX_UNROLL
        for (int c = 0; c < 3; ++c) m[3 * r + c] = (double)M[4 * r + c];
    orbx_pose_quat_from_R(m, T);
    T.tx = (double)M[3]; T.ty = (double)M[7]; T.tz = (double)M[11];
    orbx_pose_normalize(T);
    return T;
}
// Converter::toCvMat(SE3Quat): to_homogeneous_matrix narrowed to float
ORBX_HD static inline void orbx_pose_to_tcw(const OrbxPoseSE3 &T, float *M) {
    double m[9];
    orbx_pose_R_from_quat(T, m);
ORBX_UNROLL
    for (int r = 0; r < 3; ++r)
ORBX_UNROLL
        for (int c = 0; c < 3; ++c) M[4 * r + c] = (float)m[3 * r + c];
    M[3] = (float)T.tx; M[7] = (float)T.ty; M[11] = (float)T.tz;
    M[12] = 0.f; M[13] = 0.f; M[14] = 0.f; M[15] = 1.f;
}
// SE3Quat::operator*: t = a.t + a.r * b.t, r = a.r * b.r (Eigen's product), normalizeRotation
ORBX_HD static inline OrbxPoseSE3 orbx_pose_mul(const OrbxPoseSE3 &a, const OrbxPoseSE3 &b) {
    OrbxPoseSE3 r;
    double v[3];
    orbx_pose_rotate(a, b.tx, b.ty, b.tz, v);
    r.tx = a.tx + v[0]; r.ty = a.ty + v[1]; r.tz = a.tz + v[2];
    r.qw = a.qw * b.qw - a.qx * b.qx - a.qy * b.qy - a.qz * b.qz;
    r.qx = a.qw * b.qx + a.qx * b.qw + a.qy * b.qz - a.qz * b.qy;
    r.qy = a.qw * b.qy + a.qy * b.qw + a.qz * b.qx - a.qx * b.qz;
    r.qz = a.qw * b.qz + a.qz * b.qw + a.qx * b.qy - a.qy * b.qx;
    orbx_pose_normalize(r);
    return r;
}
// SE3Quat::exp(update): update = (omega, upsilon).  3x3 products sum k = 0, 1, 2 in order; R = (I + a Omega) + b Omega^2.
ORBX_HD static inline OrbxPoseSE3 orbx_pose_exp(const double *u) {
    const double o0 = u[0], o1 = u[1], o2 = u[2];
    const double theta = sqrt(o0 * o0 + o1 * o1 + o2 * o2);
    const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};
    double Om2[9], R[9], V[9];
ORBX_UNROLL
    for (int i = 0; i < 3; ++i)
ORBX_UNROLL
        for (int j = 0; j < 3; ++j) Om2[3 * i + j] = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
    if (theta < 0.00001) {
ORBX_UNROLL
        for (int i = 0; i < 9; ++i) { R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + Om[i]) + Om2[i]; V[i] = R[i]; }
    } else {
        double sn, cs;
        orbx_pose_sincos(theta, &sn, &cs);
        const double t2 = theta * theta;
        const double a = sn / theta, b = (1.0 - cs) / t2, c = (theta - sn) / (t2 * theta);
ORBX_UNROLL
        for (int i = 0; i < 9; ++i) {
            const double id = i % 4 == 0 ? 1.0 : 0.0;
            R[i] = (id + a * Om[i]) + b * Om2[i];
            V[i] = (id + b * Om[i]) + c * Om2[i];
        }
    }
    OrbxPoseSE3 T;
    orbx_pose_quat_from_R(R, T);
    T.tx = V[0] * u[3] + V[1] * u[4] + V[2] * u[5];
    T.ty = V[3] * u[3] + V[4] * u[4] + V[5] * u[5];
    T.tz = V[6] * u[3] + V[7] * u[4] + V[8] * u[5];
    orbx_pose_normalize(T);
    return T;
}

// Feature i of the view as an edge; false: no MapPoint there.  A list position outside [0, npoints) and an octave outside
// [0, nlevels) cannot be met after the host validation of host rows; device rows are not read by the host, so there the
// feature is treated as one without a point (no read leaves the pool or the level table).
ORBX_HD static inline bool orbx_pose_load(const OrbxPoseView &v, int i, OrbxPoseEdge &e) {
    const int32_t pos = v.pt[i];
    if (pos < 0 || pos >= v.npoints) return false;
    const int32_t oct = v.kp[i].octave;
    if (oct < 0 || oct >= v.nlevels) return false;
    const long long pp = v.index ? v.index[pos] : pos;
    const float ur = v.ur ? v.ur[i] : -1.0f;
    e.stereo = ur < 0 ? 0 : 1;                              // mvuRight[i] < 0: monocular edge
    e.ox = (double)v.kp[i].x; e.oy = (double)v.kp[i].y; e.our = (double)ur;
    e.w = (double)v.sig[oct];
    e.X = (double)v.world[3 * pp]; e.Y = (double)v.world[3 * pp + 1]; e.Z = (double)v.world[3 * pp + 2];
    return true;
}

// computeError + chi2 of one edge at pose T: err = obs - cam_project(T.map(Xw)); chi2 = e . (Omega e), Omega = w I, summed
// in component order.  pc receives the camera-frame point.
ORBX_HD static inline double orbx_pose_error(const OrbxPoseSE3 &T, const OrbxPoseCam &K, const OrbxPoseEdge &e, double *pc, double *err) {
    orbx_pose_rotate(T, e.X, e.Y, e.Z, pc);
    pc[0] = pc[0] + T.tx; pc[1] = pc[1] + T.ty; pc[2] = pc[2] + T.tz;
    if (e.stereo) {
        const double invz = (double)(float)(1.0 / pc[2]);     // const float invz = 1.0f / trans_xyz[2]
        const double u = pc[0] * invz * K.fx + K.cx;
        err[0] = e.ox - u;
        err[1] = e.oy - (pc[1] * invz * K.fy + K.cy);
        err[2] = e.our - (u - K.bf * invz);
        return (err[0] * (e.w * err[0]) + err[1] * (e.w * err[1])) + err[2] * (e.w * err[2]);
    }
    err[0] = e.ox - ((pc[0] / pc[2]) * K.fx + K.cx);
    err[1] = e.oy - ((pc[1] / pc[2]) * K.fy + K.cy);
    err[2] = 0.0;
    return err[0] * (e.w * err[0]) + err[1] * (e.w * err[1]);
}
// RobustKernelHuber::robustify with the edge kind's delta; without the kernel rho = (chi2, 1)
ORBX_HD static inline double orbx_pose_huber(double chi2, int stereo, bool robust, double *rho1) {
    *rho1 = 1.0;
    return robust ? orbx_lm_huber(chi2, stereo ? ORBX_POSE_DELTA_STEREO : ORBX_POSE_DELTA_MONO, rho1) : chi2;
}
// One edge's 28 terms at pose T: t[0..20] = A^T (rho1 Omega) A, upper triangle row by row; t[21..26] = rho1 (A^T Omega e);
// t[27] = rho0.  Per entry the rows are summed in order r = 0, 1[, 2]; a product is (A_rj * W) * A_rk with W = rho1 * w,
// and A_rj * (w * e_r) for b.
ORBX_HD static inline void orbx_pose_terms(const OrbxPoseSE3 &T, const OrbxPoseCam &K, const OrbxPoseEdge &e, bool robust, double *t) {
    double pc[3], err[3], rho1;
    const double chi2 = orbx_pose_error(T, K, e, pc, err);
    t[27] = orbx_pose_huber(chi2, e.stereo, robust, &rho1);
    const double x = pc[0], y = pc[1];
    const double invz = 1.0 / pc[2];
    const double invz_2 = invz * invz;
    double J[18];
    J[0] = x * y * invz_2 * K.fx;
    J[1] = -(1.0 + (x * x * invz_2)) * K.fx;
    J[2] = y * invz * K.fx;
    J[3] = -invz * K.fx;
    J[4] = 0.0;
    J[5] = x * invz_2 * K.fx;
    J[6] = (1.0 + y * y * invz_2) * K.fy;
    J[7] = -x * y * invz_2 * K.fy;
    J[8] = -x * invz * K.fy;
    J[9] = 0.0;
    J[10] = -invz * K.fy;
    J[11] = y * invz_2 * K.fy;
    J[12] = J[0] - K.bf * y * invz_2;
    J[13] = J[1] + K.bf * x * invz_2;
    J[14] = J[2];
    J[15] = J[3];
    J[16] = 0.0;
    J[17] = J[5] - K.bf * invz_2;
    const double W = rho1 * e.w;
    const double we0 = e.w * err[0], we1 = e.w * err[1], we2 = e.w * err[2];
    int n = 0;
ORBX_UNROLL
    for (int j = 0; j < 6; ++j)
ORBX_UNROLL
        for (int k = j; k < 6; ++k) {
            double s = (J[j] * W) * J[k] + (J[6 + j] * W) * J[6 + k];
            if (e.stereo) s = s + (J[12 + j] * W) * J[12 + k];
            t[n++] = s;
        }
ORBX_UNROLL
    for (int j = 0; j < 6; ++j) {
        double s = J[j] * we0 + J[6 + j] * we1;
        if (e.stereo) s = s + J[12 + j] * we2;
        t[21 + j] = rho1 * s;
    }
}

// The four rounds (src/Optimizer.cc:523-596) around SparseOptimizer::optimize(10).  The Levenberg loop stands HERE, word for word
// orbx_lm_optimize<6> of orbx_lm.h with system / chi taking the round's `robust` (tests/test_lm_parent_pin.py holds both to the
// same recorded results): behind any function boundary, forced inline included, the compilers lay out k_pose_opt and the host
// path differently, and both lose speed to it (profiles/lm_shared.md).
// Ev supplies the three passes over the edges; everything here is uniform over the lanes of a wave that run it side by side:
//   int  active()                                   number of edges of level 0
//   void system(T, robust, acc[28])                 computeActiveErrors + activeRobustChi2 + buildSystem at T, edge order
//   double chi(T, robust)                           computeActiveErrors + activeRobustChi2 at T
//   int  classify(T, Tlast)                         the inlier test: chi2 of an outlier edge at T, of every other edge at
//                                                   Tlast (where computeActiveErrors ran last); sets the flags; returns nBad
// nedges = optimizer.edges().size().  Returns nBad of the last round; *out = the estimate after it.
template <class Ev>
ORBX_HD static inline int orbx_pose_rounds(Ev &ev, const float *Tcw, int nedges, OrbxPoseSE3 *out) {
    const OrbxPoseSE3 init = orbx_pose_from_tcw(Tcw);
    OrbxPoseSE3 est = init;
    int nbad = 0;
    for (int round = 0; round < ORBX_POSE_ROUNDS; ++round) {
        est = init;                                            // setEstimate(toSE3Quat(pFrame->mTcw)): mTcw never changes
        OrbxPoseSE3 last = init;
        const bool robust = round < 3;                         // it == 2 takes the kernel off every edge
        if (ev.active() > 0) {                                 // no active edge: no active vertex, optimize() returns at once
            double lambda = 0.0, nu = 2.0;
            int stall = 0;
            for (int it = 0; it < ORBX_POSE_ITERS; ++it) {
                double acc[ORBX_POSE_TERMS], x[6];
                ev.system(est, robust, acc);
                last = est;
                double cur = acc[OrbxLm<6>::CHI];
                const double ini = cur;
                if (it == 0) {                                 // computeLambdaInit: tau * max |H_jj|, std::max as written
                    double m = 0.0;
                    int dg = 0;                                // H_jj sits 6 - j terms after H_(j-1)(j-1)
ORBX_UNROLL
                    for (int j = 0; j < 6; ++j) { const double a = __builtin_fabs(acc[dg]); m = a < m ? m : a; dg += 6 - j; }
                    lambda = 1e-5 * m;
                    nu = 2.0;
                    stall = 0;
                }
                double rho = 0.0;
                int q = 0;
                do {
                    const OrbxPoseSE3 backup = est;
                    const bool ok = orbx_lm_solve<6>(acc, lambda, acc + OrbxLm<6>::B, x);
                    est = orbx_pose_mul(orbx_pose_exp(x), est);
                    double tmp = ev.chi(est, robust);
                    last = est;
                    if (!ok) tmp = ORBX_DBL_MAX;
                    rho = cur - tmp;
                    double scale = 0.0;
ORBX_UNROLL
                    for (int j = 0; j < 6; ++j) scale = scale + x[j] * (lambda * x[j] + acc[OrbxLm<6>::B + j]);
                    scale = scale + 1e-3;
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
                        est = backup;
                    }
                    ++q;
                } while (rho < 0 && q < ORBX_LM_TRIALS);
                if (q == ORBX_LM_TRIALS || rho == 0) break;   // Terminate
                if ((ini - cur) * 1e3 < ini) ++stall; else stall = 0;
                if (stall >= 3) break;                          // Stop criterium (Raul)
            }
        }
        nbad = ev.classify(est, last);
        if (nedges < 10) break;
    }
    *out = est;
    return nbad;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side (orbx_pose.cpp, HIP-free: tests/san_pose_pack.cpp builds it alone): validation, packing, the library's host path.
// One problem as the kernel reads it
struct DPoseProb {
    int32_t frame, npoints;
    int32_t index_off;        // into the packed index array; -1: list position = pool index
    int32_t pad;
    float Tcw[16];
};
static_assert(sizeof(DPoseProb) == 80, "packed for the device");
// k_pose_opt: everything one call of orbx_pose_optimization_batch_device hands to the kernel (device pointers)
struct DPoseArgs {
    const DPoseProb *prob;
    const int32_t *index;
    const float *world, *sig;
    const orbx_keypoint *kps;
    const float *ur;             // may be NULL
    const int32_t *counts, *point;
    int cap, nlevels, nproblems;
    float fx, fy, cx, cy, mbf;
    float *Tcw;
    uint8_t *outlier;
    int32_t *ninliers;
    const float *dbg;            // NULL, or [2][nproblems][16]: est, last of orbx_debug_pose_inlier_test
};
// Uploaded block (one copy): DPoseProb[nproblems] | index[nindex] | world_pos[3 x npool] | inv_level_sigma2[nlevels]
struct OrbxPosePlan {
    int nproblems = 0;
    size_t nindex = 0;
    size_t o_prob = 0, o_index = 0, o_world = 0, o_sig = 0, o_dbg = 0, in_bytes = 0;   // o_dbg: dbg_est | dbg_last, when given
};
struct OrbxPoseCall {          // the arguments of orbx_pose_optimization_batch_device that are not per problem
    int npool = 0, nframes = 0, cap = 0, nlevels = 0;
    // orbx_debug_pose_inlier_test only: [nproblems][16] host poses; the call then runs the inlier test alone (no round)
    const float *dbg_est = nullptr, *dbg_last = nullptr;
    bool batch_form = true;   // the device batch's 16-bit feature indices bound cap; the single host call has no such limit
    const float *world_pos = nullptr, *camera4 = nullptr, *inv_level_sigma2 = nullptr;
    float mbf = 0.f;
    const orbx_keypoint *keys_un = nullptr;
    const float *u_right = nullptr;
    const int32_t *counts = nullptr, *point = nullptr;
    float *Tcw = nullptr;
    uint8_t *outlier = nullptr;
    int32_t *ninliers = nullptr;
};
// Everything the host can see, before any device work.  ORBX_OK / ORBX_BAD_ARGUMENT / ORBX_UNSUPPORTED; *why names the argument.
orbx_status orbx_pose_plan(int nproblems, const orbx_pose_problem *problems, const OrbxPoseCall &c, OrbxPosePlan &plan, const char **why);
// What only host rows allow (the host path): a list position outside a problem's list and an octave outside [0, nlevels) on a
// feature that has a point.  c's row pointers are host arrays here.
orbx_status orbx_pose_check_rows(int nproblems, const orbx_pose_problem *problems, const OrbxPoseCall &c, const char **why);
void orbx_pose_pack(const orbx_pose_problem *problems, const OrbxPoseCall &c, const OrbxPosePlan &plan, uint8_t *dst);
// The host path: the problems one after the other, c's row pointers are host arrays.  Call after the two checks.
void orbx_pose_host_run(int nproblems, const orbx_pose_problem *problems, const OrbxPoseCall &c);

