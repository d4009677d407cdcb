// orbx_sim3.h -- Sim3Solver (src/Sim3Solver.cc): ComputeSim3 (:329-454), Project (:517-541), FromCameraToImage (:550-569) and
// CheckInliers (:460-490) as scalar code shared by the host path (orbx_sim3.cpp) and the kernels (k_sim3_hypotheses,
// k_sim3_inliers).  tests/sim3_model.py restates it independently in numpy; DESIGN.md section 2 (F12) lists what was read from
// the reference's source and everything this file fixes for itself where the reference leaves it to OpenCV (cv::eigen, cv::norm,
// the MatExpr scaling, cv::Rodrigues, the order of the 3x3 float products, cv::Mat::dot) or to libm (atan2, sin, cos).
//
// fp_mode: every expression is written operation by operation and the library is built with -ffp-contract=off; the only fused
// operations are the explicit ones of orbx_pose_sincos.  ORBX_FP_GCC_FMA and ORBX_FP_STRICT handles therefore give the same
// bits, on the host and on the device.  Division and square root are the correctly rounded IEEE operations on both sides.
//
// OUTSIDE the contract (den == 0, a degenerate triple, z == 0 after a transform, non-finite input): the same code runs, every
// loop is bounded by a constant or ends on a NaN, a non-finite err compares as "not less" and the point is an outlier.
#pragma once
#include <vector>
#include "orbx_pose.h"
#include "orbx_ransac.h"

struct OrbxSim3Hyp {         // one hypothesis as the kernels store it and the host cursor reads it
    float T12[16], T21[16];  // mT12i, mT21i, row major
    float R[9], t[3], s;     // mR12i, mt12i, ms12i
    float pad[3];
};
static_assert(sizeof(OrbxSim3Hyp) == 192, "packed for the device");

enum { ORBX_SIM3_SWEEPS = 10 };
#define ORBX_SIM3_PI_HI 0x1.921fb54442d18p+1
#define ORBX_SIM3_PI_LO 0x1.1a62633145c07p-53
#define ORBX_SIM3_DBL_EPSILON 0x1p-52

// atan of q >= 0 (fdlibm's s_atan.c: argument reduction at 7/16, 11/16, 19/16, 39/16 and its degree-11 pair of polynomials),
// written with *, + and IEEE division only.  +inf gives pi/2, NaN gives NaN.
ORBX_HD static inline double orbx_sim3_atan_pos(double q) {
    int id;
    double x = q;
    if (q < 0.4375) id = -1;
    else if (q < 1.1875) {
        if (q < 0.6875) { id = 0; x = (2.0 * q - 1.0) / (2.0 + q); }
        else { id = 1; x = (q - 1.0) / (q + 1.0); }
    } else if (q < 2.4375) { id = 2; x = (q - 1.5) / (1.0 + 1.5 * q); }
    else { id = 3; x = -1.0 / q; }
    const double z = x * x;
    const double w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 +
                      w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 +
                      w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    if (id < 0) return x - x * (s1 + s2);
    const double hi = id == 0 ? 4.63647609000806093515e-01 : id == 1 ? 7.85398163397448278999e-01
                    : id == 2 ? 9.82793723247329054082e-01 : 1.57079632679489655800e+00;
    const double lo = id == 0 ? 2.26987774529616870924e-17 : id == 1 ? 3.06161699786838301793e-17
                    : id == 2 ? 1.39033110312309984516e-17 : 6.12323399573676603587e-17;
    return hi - ((x * (s1 + s2) - lo) - x);
}
// atan2(y, x) for y >= 0 (y = the norm of the quaternion's vector part): x == 0 gives 0 for y == 0 and pi/2 otherwise
ORBX_HD static inline double orbx_sim3_atan2_pos(double y, double x) {
    if (x == 0) return y == 0 ? 0.0 : 0.5 * ORBX_SIM3_PI_HI;
    const double z = orbx_sim3_atan_pos(y / __builtin_fabs(x));
    return x > 0 ? z : ORBX_SIM3_PI_HI - (z - ORBX_SIM3_PI_LO);
}

// cv::eigen of the symmetric 4x4 float matrix a (row major; only the upper triangle is read), as this library fixes it: cyclic
// Jacobi in float.  A sweep visits (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a pair with a_pq == 0 is skipped; otherwise
// theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c,
// a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq) for the two other r, and the same
// column update on V (which starts as I).  Before every sweep: off = the sum of the six squared off-diagonal entries (in the
// order above), dia = the sum of the four squared diagonal entries; the loop stops unless off > 1e-14f * dia (a NaN stops it),
// and after ORBX_SIM3_SWEEPS sweeps.  q = the column of V of the largest diagonal entry (the first on a tie), sign as computed.
// Every index below is a compile-time constant once the loops are unrolled: no per-thread array goes to scratch.
ORBX_HD static inline void orbx_sim3_eigen4(const float *N, float *q) {
    float a[4][4], v[4][4];
ORBX_UNROLL
    for (int i = 0; i < 4; ++i)
ORBX_UNROLL
        for (int j = 0; j < 4; ++j) { a[i][j] = N[4 * (i < j ? i : j) + (i < j ? j : i)]; v[i][j] = i == j ? 1.0f : 0.0f; }
    for (int sweep = 0; sweep < ORBX_SIM3_SWEEPS; ++sweep) {
        const float off = ((((a[0][1] * a[0][1] + a[0][2] * a[0][2]) + a[0][3] * a[0][3]) + a[1][2] * a[1][2]) + a[1][3] * a[1][3]) +
                          a[2][3] * a[2][3];
        const float dia = ((a[0][0] * a[0][0] + a[1][1] * a[1][1]) + a[2][2] * a[2][2]) + a[3][3] * a[3][3];
        if (!(off > 1e-14f * dia)) break;
ORBX_UNROLL
        for (int p = 0; p < 3; ++p)
ORBX_UNROLL
            for (int q_ = p + 1; q_ < 4; ++q_) {
                const float apq = a[p][q_];
                if (apq != 0.0f) {
                    const float theta = (a[q_][q_] - a[p][p]) / (2.0f * apq);
                    const float den = __builtin_fabsf(theta) + sqrtf(theta * theta + 1.0f);
                    const float t = (theta < 0.0f ? -1.0f : 1.0f) / den;
                    const float c = 1.0f / sqrtf(t * t + 1.0f);
                    const float s = t * c;
                    const float h = t * apq;
                    a[p][p] = a[p][p] - h;
                    a[q_][q_] = a[q_][q_] + h;
                    a[p][q_] = 0.0f; a[q_][p] = 0.0f;
ORBX_UNROLL
                    for (int r = 0; r < 4; ++r) {
                        if (r != p && r != q_) {
                            const float arp = a[r][p], arq = a[r][q_];
                            const float np_ = c * arp - s * arq, nq_ = s * arp + c * arq;
                            a[r][p] = np_; a[p][r] = np_;
                            a[r][q_] = nq_; a[q_][r] = nq_;
                        }
                        const float vrp = v[r][p], vrq = v[r][q_];
                        v[r][p] = c * vrp - s * vrq;
                        v[r][q_] = s * vrp + c * vrq;
                    }
                }
            }
    }
    float best = a[0][0];
    q[0] = v[0][0]; q[1] = v[1][0]; q[2] = v[2][0]; q[3] = v[3][0];
ORBX_UNROLL
    for (int k = 1; k < 4; ++k)
        if (a[k][k] > best) { best = a[k][k]; q[0] = v[0][k]; q[1] = v[1][k]; q[2] = v[2][k]; q[3] = v[3][k]; }
}

// cv::Rodrigues of the float rotation vector r, as this library fixes it: in double, theta = sqrt((rx^2 + ry^2) + rz^2),
// theta < DBL_EPSILON gives I, otherwise u = r / theta and R_ij = (c d_ij + ((1 - c) u_i) u_j) + s [u]x_ij; rounded to float.
ORBX_HD static inline void orbx_sim3_rodrigues(const float *r, float *R) {
    const double rx = (double)r[0], ry = (double)r[1], rz = (double)r[2];
    const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
    if (theta < ORBX_SIM3_DBL_EPSILON) {
ORBX_UNROLL
        for (int i = 0; i < 9; ++i) R[i] = i % 4 == 0 ? 1.0f : 0.0f;
        return;
    }
    double sn, cs;
    orbx_pose_sincos(theta, &sn, &cs);
    const double u[3] = {rx / theta, ry / theta, rz / theta};
    const double c1 = 1.0 - cs;
    const double K[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
ORBX_UNROLL
    for (int i = 0; i < 3; ++i)
ORBX_UNROLL
        for (int j = 0; j < 3; ++j)
            R[3 * i + j] = (float)(((i == j ? cs : 0.0) + (c1 * u[i]) * u[j]) + sn * K[3 * i + j]);
}

// Sim3Solver::ComputeSim3: P1, P2 are the three points of each set, point i at P[3 i .. 3 i + 2] (the columns of the source's
// 3x3 matrices).  Every 3x3 float product sums k = 0, 1, 2 in order, each product and each sum rounded to float.
ORBX_HD static inline void orbx_sim3_compute(const float *P1, const float *P2, int fix_scale, OrbxSim3Hyp &H) {
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];   // Pr[row][col]: coordinate row of point col, as the source's matrices
ORBX_UNROLL
    for (int r = 0; r < 3; ++r) {               // cv::reduce(P, C, 1, CV_REDUCE_SUM): the columns in order; C = C / P.cols
        O1[r] = ((P1[r] + P1[3 + r]) + P1[6 + r]) / 3.0f;
        O2[r] = ((P2[r] + P2[3 + r]) + P2[6 + r]) / 3.0f;
ORBX_UNROLL
        for (int c = 0; c < 3; ++c) { Pr1[r][c] = P1[3 * c + r] - O1[r]; Pr2[r][c] = P2[3 * c + r] - O2[r]; }
    }
    float M[3][3];                              // M = Pr2 * Pr1.t()
ORBX_UNROLL
    for (int i = 0; i < 3; ++i)
ORBX_UNROLL
        for (int j = 0; j < 3; ++j) M[i][j] = (Pr2[i][0] * Pr1[j][0] + Pr2[i][1] * Pr1[j][1]) + Pr2[i][2] * Pr1[j][2];
    const double m00 = (double)M[0][0], m01 = (double)M[0][1], m02 = (double)M[0][2], m10 = (double)M[1][0], m11 = (double)M[1][1],
                 m12 = (double)M[1][2], m20 = (double)M[2][0], m21 = (double)M[2][1], m22 = (double)M[2][2];
    const float N11 = (float)((m00 + m11) + m22), N12 = (float)(m12 - m21), N13 = (float)(m20 - m02), N14 = (float)(m01 - m10);
    const float N22 = (float)((m00 - m11) - m22), N23 = (float)(m01 + m10), N24 = (float)(m20 + m02);
    const float N33 = (float)((-m00 + m11) - m22), N34 = (float)(m12 + m21), N44 = (float)((-m00 - m11) + m22);
    const float N[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    float q[4];
    orbx_sim3_eigen4(N, q);
    // cv::norm(vec): squares summed in double in index order, IEEE sqrt; ang = atan2(norm, q0); vec = 2 * ang * vec / norm(vec)
    // as ONE double factor (2 ang) / norm, each product rounded to float
    const double v0 = (double)q[1], v1 = (double)q[2], v2 = (double)q[3];
    const double nv = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    const double ang = orbx_sim3_atan2_pos(nv, (double)q[0]);
    const double f = (2.0 * ang) / nv;
    const float rv[3] = {(float)(f * v0), (float)(f * v1), (float)(f * v2)};
    orbx_sim3_rodrigues(rv, H.R);
    const float *R = H.R;
    float P3[3][3];                             // P3 = mR12i * Pr2
ORBX_UNROLL
    for (int i = 0; i < 3; ++i)
ORBX_UNROLL
        for (int j = 0; j < 3; ++j) P3[i][j] = (R[3 * i] * Pr2[0][j] + R[3 * i + 1] * Pr2[1][j]) + R[3 * i + 2] * Pr2[2][j];
    float s = 1.0f;
    if (!fix_scale) {                           // cv::Mat::dot: products of the widened floats summed in double, row major
        double nom = 0.0, den = 0.0;
ORBX_UNROLL
        for (int i = 0; i < 3; ++i)
ORBX_UNROLL
            for (int j = 0; j < 3; ++j) {
                nom = nom + (double)Pr1[i][j] * (double)P3[i][j];
                den = den + (double)(P3[i][j] * P3[i][j]);   // cv::pow(P3, 2, aux_P3) is a float matrix
            }
        s = (float)(nom / den);
    }
    H.s = s;
    float sR[9], sRi[9];
    const double inv = 1.0 / (double)s;         // (1.0 / ms12i) * mR12i.t(): one double factor, each product rounded to float
ORBX_UNROLL
    for (int i = 0; i < 3; ++i)
ORBX_UNROLL
        for (int j = 0; j < 3; ++j) { sR[3 * i + j] = s * R[3 * i + j]; sRi[3 * i + j] = (float)(inv * (double)R[3 * j + i]); }
ORBX_UNROLL
    for (int i = 0; i < 3; ++i)                 // mt12i = O1 - ms12i * mR12i * O2
        H.t[i] = O1[i] - ((sR[3 * i] * O2[0] + sR[3 * i + 1] * O2[1]) + sR[3 * i + 2] * O2[2]);
ORBX_UNROLL
    for (int i = 0; i < 3; ++i) {
ORBX_UNROLL
        for (int j = 0; j < 3; ++j) { H.T12[4 * i + j] = sR[3 * i + j]; H.T21[4 * i + j] = sRi[3 * i + j]; }
        H.T12[4 * i + 3] = H.t[i];
        H.T21[4 * i + 3] = -((sRi[3 * i] * H.t[0] + sRi[3 * i + 1] * H.t[1]) + sRi[3 * i + 2] * H.t[2]);   // tinv = -sRinv * mt12i
        H.T12[12 + i] = 0.0f; H.T21[12 + i] = 0.0f;
    }
    H.T12[15] = 1.0f; H.T21[15] = 1.0f;
ORBX_UNROLL
    for (int i = 0; i < 12; ++i) { H.T12[i] = orbx_canonf(H.T12[i]); H.T21[i] = orbx_canonf(H.T21[i]); }
ORBX_UNROLL
    for (int i = 0; i < 9; ++i) H.R[i] = orbx_canonf(H.R[i]);
ORBX_UNROLL
    for (int i = 0; i < 3; ++i) H.t[i] = orbx_canonf(H.t[i]);
    H.s = orbx_canonf(H.s);
    H.pad[0] = 0.0f; H.pad[1] = 0.0f; H.pad[2] = 0.0f;
}

// FromCameraToImage of one point: invz = 1 / z, (fx (X invz) + cx, fy (Y invz) + cy); K = fx, fy, cx, cy
ORBX_HD static inline void orbx_sim3_to_image(float X, float Y, float Z, const float *K, float *u, float *v) {
    const float invz = 1.0f / Z;
    const float x = X * invz, y = Y * invz;
    *u = K[0] * x + K[2];
    *v = K[1] * y + K[3];
}
// Project of one point: P3Dc = Rcw * X + tcw (row sums k = 0, 1, 2, then + t), then FromCameraToImage
ORBX_HD static inline void orbx_sim3_project(const float *T, float X, float Y, float Z, const float *K, float *u, float *v) {
    const float x = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
    const float y = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
    const float z = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
    orbx_sim3_to_image(x, y, z, K, u, v);
}
// dist.dot(dist) of a 2-vector (cv::Mat::dot: widened products summed in double), stored as float
ORBX_HD static inline float orbx_sim3_err(float ax, float ay, float bx, float by) {
    const float dx = ax - bx, dy = ay - by;
    return (float)((double)dx * (double)dx + (double)dy * (double)dy);
}
// CheckInliers for one correspondence: x1, x2 = mvX3Dc1[i], mvX3Dc2[i]; p1, p2 = mvP1im1[i], mvP2im2[i]
ORBX_HD static inline bool orbx_sim3_inlier(const float *T12, const float *T21, const float *K1, const float *K2, const float *x1,
                                            const float *x2, const float *p1, const float *p2, float max1, float max2) {
    float u21, v21, u12, v12;
    orbx_sim3_project(T12, x2[0], x2[1], x2[2], K1, &u21, &v21);   // vP2im1
    orbx_sim3_project(T21, x1[0], x1[1], x1[2], K2, &u12, &v12);   // vP1im2
    const float err1 = orbx_sim3_err(p1[0], p1[1], u21, v21);      // dist1 = mvP1im1[i] - vP2im1[i]
    const float err2 = orbx_sim3_err(u12, v12, p2[0], p2[1]);      // dist2 = vP1im2[i] - mvP2im2[i]
    return err1 < max1 && err2 < max2;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side (orbx_sim3.cpp, HIP-free: tests/san_sim3.cpp builds it alone): validation, packing, the host path, the cursor.
enum { ORBX_SIM3_PLANES = 12,       // per correspondence: X1c (3) | X2c (3) | max_err1 | max_err2 | P1im1 (2) | P2im2 (2)
       ORBX_SIM3_WAVES = 4,         // waves (iterations) per workgroup of k_sim3_inliers
       ORBX_SIM3_CHUNK = 512 };     // correspondences staged in LDS at a time (24 KiB)
struct DSim3Prob {                  // one problem that launches, as the kernels read it
    int32_t n, iterations, fix_scale, nwords;   // nwords = ceil(n / 64)
    int32_t iter_off;               // first hypothesis / count of the problem
    int32_t pts_off;                // first float of its ORBX_SIM3_PLANES planes of n floats
    int32_t word_off;               // first mask word: [iterations][nwords]
    int32_t pad;
    float K1[4], K2[4];
};
static_assert(sizeof(DSim3Prob) == 64, "packed for the device");
// sets: [total_hyps][3]; a group: ORBX_SIM3_WAVES iterations of k_sim3_inliers; tally: the inlier counts
using DSim3Args = DRansacArgs<DSim3Prob, OrbxSim3Hyp, int32_t>;
using OrbxSim3Plan = OrbxRansacPlan;
orbx_status orbx_sim3_plan(int nproblems, const orbx_sim3_problem *problems, OrbxSim3Plan &plan, const char **why);
void orbx_sim3_pack(const orbx_sim3_problem *problems, const OrbxSim3Plan &plan, uint8_t *dst);
// the host path: reads the packed block, writes the downloaded block's layout (hyp | masks | counts) into out
void orbx_sim3_host_run(const OrbxSim3Plan &plan, const uint8_t *in, uint8_t *out);

struct OrbxSim3State {              // one solver of a batch: what iterate() keeps between calls
    int32_t n = 0, min_inliers = 0, iterations = 0, nwords = 0;
    int32_t iter_off = -1;          // -1: n < min_inliers, nothing was computed
    size_t word_off = 0;
    int32_t done = 0, best_inliers = 0, best_it = -1;   // mnIterations, mnBestInliers, the hypothesis behind mBest*
};
struct orbx_sim3_batch {
    std::vector<OrbxSim3State> st;
    std::vector<uint8_t> out;       // hyp | masks | counts
    size_t o_hyp = 0, o_masks = 0, o_counts = 0;
};
orbx_sim3_batch *orbx_sim3_batch_new(const orbx_sim3_problem *problems, const OrbxSim3Plan &plan);   // out zeroed, states at start
void orbx_sim3_batch_take(orbx_sim3_batch *b, const OrbxSim3Plan &plan, const uint8_t *out);         // the downloaded block, copied
// The cursor behind orbx_sim3_batch_iterate / _best / _counts / _hypothesis; *why names what was wrong
int32_t orbx_sim3_cursor_iterate(orbx_sim3_batch *b, int k, int n_iterations, int32_t *no_more, uint8_t *inliers, int32_t *ninliers,
                                 float *T12, const char **why);
orbx_status orbx_sim3_cursor_best(const orbx_sim3_batch *b, int k, float *R, float *t, float *s, const char **why);
orbx_status orbx_sim3_cursor_counts(const orbx_sim3_batch *b, int k, int32_t *counts, int32_t *niterations, const char **why);
orbx_status orbx_sim3_cursor_hypothesis(const orbx_sim3_batch *b, int k, int iteration, float *hyp48, uint64_t *mask_words,
                                        const char **why);
