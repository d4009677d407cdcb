// orbx_newpoints.h -- the per-match geometry of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:450-651) with
// KeyFrame::UnprojectStereo (src/KeyFrame.cc:937-958) as scalar code shared by the host path (orbx_newpoints.cpp) and the kernel
// (k_new_points).  tests/newpoints_model.py restates it independently in numpy; DESIGN.md section 2 (F17) lists what was read
// from the reference's source and everything this file fixes for itself where the reference leaves it to OpenCV or libm
// (cv::SVD::compute, cv::norm, Mat::dot, the matrix products, Mat / scalar, atan2f, cosf).
//
// fp_mode: every expression is written operation by operation and the library is built with -ffp-contract=off, so
// ORBX_FP_GCC_FMA and ORBX_FP_STRICT handles give the same bits, on the host and on the device.  Division and square root are the
// correctly rounded IEEE operations on both sides.  No math library is called: atan2f is orbx_sim3_atan2_pos rounded to float,
// cosf is orbx_sincosf_pinned.
//
// Registers: the 4 x 4 system and its V are a float[32] of orbx_newpoints_match's own and every index into it is a constant once
// the loops are unrolled (as in orbx_recon_check_match), so k_new_points uses neither LDS nor scratch.
//
// Non-finite input runs the same straight-line code, every loop is bounded by a constant, a comparison with a NaN is false
// wherever the source compares, and a NaN that is stored is stored as the canonical quiet NaN.
#pragma once
#include <vector>
#include "orbx_recon.h"
#include "orbx_sim3.h"
#include "orbx_sincos.h"

enum { ORBX_NEWPTS_CHUNK = 64,          // matches (lanes) per workgroup of k_new_points: one wave
       ORBX_NEWPTS_PLANES = 16 };       // per match, gathered by the host: see OrbxNewPtsPlane
enum OrbxNewPtsPlane { NP_UX1, NP_UY1, NP_UX2, NP_UY2,       // mvKeysUn[idx].pt
                       NP_KX1, NP_KY1, NP_KX2, NP_KY2,       // mvKeys[idx].pt
                       NP_UR1, NP_UR2, NP_D1, NP_D2,         // mvuRight[idx], mvDepth[idx]
                       NP_SIG1, NP_SIG2, NP_SC1, NP_SC2 };   // mvLevelSigma2[octave], mvScaleFactors[octave]

struct DNewPtsCam {                     // one keyframe of a problem as the kernel reads it (wave-uniform)
    float Rcw[9], tcw[3], Ow[3];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
    float pad;
};
static_assert(sizeof(DNewPtsCam) == 96, "packed for the device");
struct DNewPtsProb {
    DNewPtsCam c1, c2;
    float ratio_factor;                 // 1.5f * mfScaleFactor of KF1
    int32_t n;                          // matches
    int32_t m_off;                      // first match: plane entry, status byte, point m_off (fits: the plan bounds the total)
    int32_t pad[13];
};
static_assert(sizeof(DNewPtsProb) == 256, "packed for the device");
struct DNewPtsChunk { int32_t prob, base; };   // one workgroup: matches base .. base + 63 of problem prob

struct OrbxNewPtsObs { float ux, uy, kx, ky, ur, depth, sigma2, scale; };   // one side of a match

// cos(2 * atan2(mb / 2, depth)) of :492 / :495 for depth > 0.  With <cmath> and the `using namespace std` the reference's headers
// bring in (DBoW2's TemplatedVocabulary.h), the unqualified atan2(float, float) and cos(float) resolve to the float overloads:
// mb / 2 is a float, atan2f returns a float, 2 * that is a float product, cosf returns a float.  atan2f as this library fixes it:
// orbx_sim3_atan2_pos of the two floats in double, rounded to float once.  Its y is |mb / 2|: atan2 is odd in y and cos is even,
// so the value is that of the signed argument.  cosf: orbx_sincosf_pinned, the angle is in (0, pi).
ORBX_HD static inline float orbx_newpoints_stereo_cosf(float mb, float depth) {
    const float y = __builtin_fabsf(mb / 2.0f);
    const float a = (float)orbx_sim3_atan2_pos((double)y, (double)depth);
    const float ang = 2.0f * a;
    return orbx_sincosf_pinned(ang).c;
}
// Mat::dot of a row of Rcw with x3Dt (the rule of F15: products and sum in double, index order) + the float entry of tcw, which
// the source adds in double before the assignment rounds to float
ORBX_HD static inline float orbx_newpoints_row(const float *r, float t, float X, float Y, float Z) {
    const double dot = ((double)r[0] * (double)X + (double)r[1] * (double)Y) + (double)r[2] * (double)Z;
    return (float)(dot + (double)t);
}
// KeyFrame::UnprojectStereo for z > 0: the DISTORTED keypoint, (u - cx) * z * invfx in that order, Twc = [Rcw^T | Ow]:
// each entry ((Rwc_i0 x + Rwc_i1 y) + Rwc_i2 z) + Ow_i in float
ORBX_HD static inline void orbx_newpoints_unproject(const DNewPtsCam &C, const OrbxNewPtsObs &o, float *X) {
    const float z = o.depth;
    const float x = (o.kx - C.cx) * z * C.invfx;
    const float y = (o.ky - C.cy) * z * C.invfy;
ORBX_UNROLL
    for (int i = 0; i < 3; ++i) X[i] = ((C.Rcw[i] * x + C.Rcw[3 + i] * y) + C.Rcw[6 + i] * z) + C.Ow[i];
}
// One reprojection test (:571-596 / :604-623): true = `continue`.  mbf is KF1's in both keyframes (:616).
ORBX_HD static inline bool orbx_newpoints_reproj_fails(const DNewPtsCam &C, float mbf, const OrbxNewPtsObs &o, bool stereo, float x,
                                                       float y, float z) {
    const float invz = 1.0f / z;                                 // 1.0 / z to float: the same value (orbx_init.h)
    const float u = C.fx * x * invz + C.cx;
    const float v = C.fy * y * invz + C.cy;
    const float errX = u - o.ux, errY = v - o.uy;
    if (!stereo) return (double)(errX * errX + errY * errY) > 5.991 * (double)o.sigma2;
    const float u_r = u - mbf * invz;
    const float errX_r = u_r - o.ur;
    return (double)((errX * errX + errY * errY) + errX_r * errX_r) > 7.8 * (double)o.sigma2;
}

// One match of the loop body: returns the status byte (ORBX_NEWPOINT_*) and the point (zeros for every rejecting status).
ORBX_HD static inline int orbx_newpoints_match(const DNewPtsCam &C1, const DNewPtsCam &C2, float ratioFactor, const OrbxNewPtsObs &o1,
                                               const OrbxNewPtsObs &o2, float *pt) {
    pt[0] = 0.0f; pt[1] = 0.0f; pt[2] = 0.0f;
    const bool bStereo1 = o1.ur >= 0.0f, bStereo2 = o2.ur >= 0.0f;
    if ((bStereo1 && !(o1.depth > 0.0f)) || (bStereo2 && !(o2.depth > 0.0f))) return ORBX_NEWPOINT_NO_DEPTH;
    const float xn1x = (o1.ux - C1.cx) * C1.invfx, xn1y = (o1.uy - C1.cy) * C1.invfy;
    const float xn2x = (o2.ux - C2.cx) * C2.invfx, xn2y = (o2.uy - C2.cy) * C2.invfy;
    float ray1[3], ray2[3];                                      // Rwc * xn, Rwc = Rcw^T, xn(2) = 1
ORBX_UNROLL
    for (int i = 0; i < 3; ++i) {
        ray1[i] = (C1.Rcw[i] * xn1x + C1.Rcw[3 + i] * xn1y) + C1.Rcw[6 + i];
        ray2[i] = (C2.Rcw[i] * xn2x + C2.Rcw[3 + i] * xn2y) + C2.Rcw[6 + i];
    }
    const double dot = ((double)ray1[0] * (double)ray2[0] + (double)ray1[1] * (double)ray2[1]) + (double)ray1[2] * (double)ray2[2];
    const float cosParallaxRays =
        (float)(dot / (orbx_recon_norm3(ray1[0], ray1[1], ray1[2]) * orbx_recon_norm3(ray2[0], ray2[1], ray2[2])));
    float cosParallaxStereo = cosParallaxRays + 1.0f;
    float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = orbx_newpoints_stereo_cosf(C1.mb, o1.depth);
    else if (bStereo2) cosParallaxStereo2 = orbx_newpoints_stereo_cosf(C2.mb, o2.depth);
    cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   // std::min(a, b)
    float X[3];
    int status;
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0.0f && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
        float ws[32];
        const OrbxInitWs W = {ws, 1};
ORBX_UNROLL
        for (int j = 0; j < 4; ++j) {                            // rows of Tcw = [Rcw | tcw], not of K [R | t]
            const float a0 = j < 3 ? C1.Rcw[j] : C1.tcw[0], a1 = j < 3 ? C1.Rcw[3 + j] : C1.tcw[1], a2 = j < 3 ? C1.Rcw[6 + j] : C1.tcw[2];
            const float b0 = j < 3 ? C2.Rcw[j] : C2.tcw[0], b1 = j < 3 ? C2.Rcw[3 + j] : C2.tcw[1], b2 = j < 3 ? C2.Rcw[6 + j] : C2.tcw[2];
            ws[j] = xn1x * a2 - a0;
            ws[4 + j] = xn1y * a2 - a1;
            ws[8 + j] = xn2x * b2 - b0;
            ws[12 + j] = xn2y * b2 - b1;
        }
        const int col = orbx_init_jacobi(W, 0, 16, 4, 4);
        float x[4];
ORBX_UNROLL
        for (int i = 0; i < 4; ++i)
            x[i] = col == 0 ? ws[16 + 4 * i] : col == 1 ? ws[17 + 4 * i] : col == 2 ? ws[18 + 4 * i] : ws[19 + 4 * i];
        if (x[3] == 0.0f) return ORBX_NEWPOINT_ZERO_W;
        X[0] = x[0] / x[3]; X[1] = x[1] / x[3]; X[2] = x[2] / x[3];
        status = ORBX_NEWPOINT_TRIANGULATED;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        orbx_newpoints_unproject(C1, o1, X);
        status = ORBX_NEWPOINT_STEREO1;
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        orbx_newpoints_unproject(C2, o2, X);
        status = ORBX_NEWPOINT_STEREO2;
    } else
        return ORBX_NEWPOINT_LOW_PARALLAX;
    const float z1 = orbx_newpoints_row(C1.Rcw + 6, C1.tcw[2], X[0], X[1], X[2]);
    if (z1 <= 0.0f) return ORBX_NEWPOINT_DEPTH1;
    const float z2 = orbx_newpoints_row(C2.Rcw + 6, C2.tcw[2], X[0], X[1], X[2]);
    if (z2 <= 0.0f) return ORBX_NEWPOINT_DEPTH2;
    const float x1 = orbx_newpoints_row(C1.Rcw, C1.tcw[0], X[0], X[1], X[2]);
    const float y1 = orbx_newpoints_row(C1.Rcw + 3, C1.tcw[1], X[0], X[1], X[2]);
    if (orbx_newpoints_reproj_fails(C1, C1.mbf, o1, bStereo1, x1, y1, z1)) return ORBX_NEWPOINT_REPROJ1;
    const float x2 = orbx_newpoints_row(C2.Rcw, C2.tcw[0], X[0], X[1], X[2]);
    const float y2 = orbx_newpoints_row(C2.Rcw + 3, C2.tcw[1], X[0], X[1], X[2]);
    if (orbx_newpoints_reproj_fails(C2, C1.mbf, o2, bStereo2, x2, y2, z2)) return ORBX_NEWPOINT_REPROJ2;
    const float dist1 = (float)orbx_recon_norm3(X[0] - C1.Ow[0], X[1] - C1.Ow[1], X[2] - C1.Ow[2]);
    const float dist2 = (float)orbx_recon_norm3(X[0] - C2.Ow[0], X[1] - C2.Ow[1], X[2] - C2.Ow[2]);
    if (dist1 == 0.0f || dist2 == 0.0f) return ORBX_NEWPOINT_ZERO_DIST;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = o1.scale / o2.scale;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return ORBX_NEWPOINT_SCALE;
    pt[0] = orbx_canonf(X[0]); pt[1] = orbx_canonf(X[1]); pt[2] = orbx_canonf(X[2]);
    return status;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side (orbx_newpoints.cpp, HIP-free): validation, packing (the gather by index), the host path, the scatter.
// Uploaded block (one copy): DNewPtsProb[nproblems] | DNewPtsChunk[nchunks] | ORBX_NEWPTS_PLANES planes of total floats (plane p,
// match g of the call at p * total + g).  Downloaded block: status[total] | points[total][3].
struct OrbxNewPtsPlan {
    int nproblems = 0, nchunks = 0;
    size_t total = 0;
    size_t o_prob = 0, o_chunk = 0, o_planes = 0, in_bytes = 0;
    size_t o_st = 0, o_pts = 0, out_bytes = 0;
};
struct DNewPtsArgs {                    // what the kernel gets, by value
    const DNewPtsProb *prob; const DNewPtsChunk *chunk; const float *planes;
    uint8_t *st; float *pts;
    int nchunks, total;
};
static inline DNewPtsArgs orbx_newpoints_args(const OrbxNewPtsPlan &p, uint8_t *in, uint8_t *out) {
    DNewPtsArgs a;
    a.prob = (const DNewPtsProb *)(in + p.o_prob); a.chunk = (const DNewPtsChunk *)(in + p.o_chunk);
    a.planes = (const float *)(in + p.o_planes);
    a.st = out + p.o_st; a.pts = (float *)(out + p.o_pts);
    a.nchunks = p.nchunks; a.total = (int)p.total;
    return a;
}
// one side of match g of the call from the planes
ORBX_HD static inline OrbxNewPtsObs orbx_newpoints_obs(const float *planes, long long total, long long g, int side) {
    OrbxNewPtsObs o;
    o.ux = planes[(NP_UX1 + 2 * side) * total + g]; o.uy = planes[(NP_UY1 + 2 * side) * total + g];
    o.kx = planes[(NP_KX1 + 2 * side) * total + g]; o.ky = planes[(NP_KY1 + 2 * side) * total + g];
    o.ur = planes[(NP_UR1 + side) * total + g]; o.depth = planes[(NP_D1 + side) * total + g];
    o.sigma2 = planes[(NP_SIG1 + side) * total + g]; o.scale = planes[(NP_SC1 + side) * total + g];
    return o;
}
orbx_status orbx_newpoints_plan(int nproblems, const orbx_newpoints_problem *problems, const uint8_t *status_out,
                                const float *points_out, OrbxNewPtsPlan &plan, const char **why);
void orbx_newpoints_pack(const orbx_newpoints_problem *problems, const OrbxNewPtsPlan &plan, uint8_t *dst);
// the host path: reads the packed block, writes the downloaded block's layout into out
void orbx_newpoints_host_run(const OrbxNewPtsPlan &plan, const uint8_t *in, uint8_t *out);
void orbx_newpoints_unpack(const OrbxNewPtsPlan &plan, const uint8_t *out, uint8_t *status_out, float *points_out);
