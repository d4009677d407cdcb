// orbx_pose.cpp -- host side of the batched Optimizer::PoseOptimization (orbx_pose.h): validation of a call, the packing of all
// problems' small host state into one staging block, and the library's host path -- the header's scalar code compiled by the
// host compiler, the problems one after the other and the edges of a problem in feature order.  HIP-free:
// tests/san_pose_pack.cpp builds it alone under the sanitizers.  The entry points (orbx_map_batches.cpp) own the staging block, the
// arena and the launch.
#include <cstring>
#include "orbx_pose.h"
#include "orbx_ransac.h"   // orbx_pad256

orbx_status orbx_pose_plan(int nproblems, const orbx_pose_problem *problems, const OrbxPoseCall &c, OrbxPosePlan &plan, const char **why) {
    plan = OrbxPosePlan();
    if (nproblems < 0) { *why = "nproblems < 0"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !problems) { *why = "null problem array"; return ORBX_BAD_ARGUMENT; }
    if (c.cap <= 0) { *why = "cap <= 0"; return ORBX_BAD_ARGUMENT; }
    if (c.batch_form && c.cap > 65535) { *why = "cap > 65535 (feature indices are 16-bit in the device batch)"; return ORBX_UNSUPPORTED; }
    if (nproblems == 0) return ORBX_OK;
    if (c.nframes <= 0) { *why = "nframes <= 0"; return ORBX_BAD_ARGUMENT; }
    if (c.npool < 0) { *why = "npool < 0"; return ORBX_BAD_ARGUMENT; }
    if (c.nlevels < 1) { *why = "nlevels < 1"; return ORBX_BAD_ARGUMENT; }
    if (!c.keys_un || !c.counts || !c.point || !c.Tcw || !c.outlier || !c.ninliers) { *why = "null frame or result buffer"; return ORBX_BAD_ARGUMENT; }
    if (!c.camera4 || !c.inv_level_sigma2) { *why = "null camera4 or inv_level_sigma2"; return ORBX_BAD_ARGUMENT; }
    if ((c.dbg_est == nullptr) != (c.dbg_last == nullptr)) { *why = "one of the two debug poses is null"; return ORBX_BAD_ARGUMENT; }
    if (c.npool > 0 && !c.world_pos) { *why = "null world_pos with a non-empty pool"; return ORBX_BAD_ARGUMENT; }
    size_t nindex = 0;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_pose_problem &P = problems[k];
        if (P.frame < 0 || P.frame >= c.nframes) { *why = "frame outside [0, nframes)"; return ORBX_BAD_ARGUMENT; }
        if (P.npoints < 0) { *why = "npoints < 0"; return ORBX_BAD_ARGUMENT; }
        if (P.point_index) {
            for (int i = 0; i < P.npoints; ++i)
                if (P.point_index[i] < 0 || P.point_index[i] >= c.npool) { *why = "point_index outside the pool"; return ORBX_BAD_ARGUMENT; }
            nindex += (size_t)P.npoints;
        } else if (P.npoints > c.npool) {
            *why = "point_index is NULL and npoints exceeds the pool";
            return ORBX_BAD_ARGUMENT;
        }
    }
    if (nindex > (size_t)0x7fffffff) { *why = "too many points for 32-bit offsets"; return ORBX_UNSUPPORTED; }
    plan.nproblems = nproblems;
    plan.nindex = nindex;
    plan.o_prob = 0;
    plan.o_index = orbx_pad256((size_t)nproblems * sizeof(DPoseProb));
    plan.o_world = plan.o_index + orbx_pad256(nindex * sizeof(int32_t));
    plan.o_sig = plan.o_world + orbx_pad256((size_t)c.npool * 3 * sizeof(float));
    plan.o_dbg = plan.o_sig + orbx_pad256((size_t)c.nlevels * sizeof(float));
    plan.in_bytes = plan.o_dbg + (c.dbg_est ? orbx_pad256((size_t)nproblems * 32 * sizeof(float)) : 0);
    return ORBX_OK;
}

orbx_status orbx_pose_check_rows(int nproblems, const orbx_pose_problem *problems, const OrbxPoseCall &c, const char **why) {
    for (int k = 0; k < nproblems; ++k) {
        const orbx_pose_problem &P = problems[k];
        const int cnt = c.counts[P.frame];
        const int n = cnt < 0 ? 0 : cnt < c.cap ? cnt : c.cap;
        const int32_t *pt = c.point + (size_t)k * c.cap;
        const orbx_keypoint *kp = c.keys_un + (size_t)P.frame * c.cap;
        for (int i = 0; i < n; ++i) {
            if (pt[i] < 0) continue;
            if (pt[i] >= P.npoints) { *why = "point row names a position outside the problem's list"; return ORBX_BAD_ARGUMENT; }
            if (kp[i].octave < 0 || kp[i].octave >= c.nlevels) {
                *why = "octave outside [0, nlevels) on a feature with a MapPoint";
                return ORBX_BAD_ARGUMENT;
            }
        }
    }
    return ORBX_OK;
}

void orbx_pose_pack(const orbx_pose_problem *problems, const OrbxPoseCall &c, const OrbxPosePlan &plan, uint8_t *dst) {
    if (plan.nproblems <= 0) return;
    DPoseProb *dp = (DPoseProb *)(dst + plan.o_prob);
    int32_t *index = (int32_t *)(dst + plan.o_index);
    size_t off = 0;
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_pose_problem &P = problems[k];
        DPoseProb &D = dp[k];
        D.frame = P.frame; D.npoints = P.npoints; D.pad = 0;
        D.index_off = -1;
        if (P.point_index) {
            D.index_off = (int32_t)off;
            if (P.npoints > 0) memcpy(index + off, P.point_index, (size_t)P.npoints * sizeof(int32_t));
            off += (size_t)P.npoints;
        }
        memcpy(D.Tcw, P.Tcw, sizeof(D.Tcw));
    }
    if (c.npool > 0) memcpy(dst + plan.o_world, c.world_pos, (size_t)c.npool * 3 * sizeof(float));
    memcpy(dst + plan.o_sig, c.inv_level_sigma2, (size_t)c.nlevels * sizeof(float));
    if (c.dbg_est) {
        const size_t b = (size_t)plan.nproblems * 16 * sizeof(float);
        memcpy(dst + plan.o_dbg, c.dbg_est, b);
        memcpy(dst + plan.o_dbg + b, c.dbg_last, b);
    }
}

namespace {
// The three passes of orbx_pose_rounds over one problem's edges, one edge after the other
struct PoseEvHost {
    OrbxPoseView v;
    OrbxPoseCam K;
    uint8_t *outlier;
    int nactive;
    int active() const { return nactive; }
    void system(const OrbxPoseSE3 &T, bool robust, double *acc) const {
        for (int t = 0; t < ORBX_POSE_TERMS; ++t) acc[t] = 0.0;
        OrbxPoseEdge e;
        double term[ORBX_POSE_TERMS];
        for (int i = 0; i < v.n; ++i) {
            if (!orbx_pose_load(v, i, e) || outlier[i]) continue;
            orbx_pose_terms(T, K, e, robust, term);
            for (int t = 0; t < ORBX_POSE_TERMS; ++t) acc[t] = orbx_lm_accumulate<6>(t, acc[t], term[t]);
        }
    }
    double chi(const OrbxPoseSE3 &T, bool robust) const {
        double s = 0.0, pc[3], err[3], rho1;
        OrbxPoseEdge e;
        for (int i = 0; i < v.n; ++i) {
            if (!orbx_pose_load(v, i, e) || outlier[i]) continue;
            s = s + orbx_pose_huber(orbx_pose_error(T, K, e, pc, err), e.stereo, robust, &rho1);
        }
        return s;
    }
    int classify(const OrbxPoseSE3 &T, const OrbxPoseSE3 &Tlast) {
        int nbad = 0;
        nactive = 0;
        double pc[3], err[3];
        OrbxPoseEdge e;
        for (int i = 0; i < v.n; ++i) {
            if (!orbx_pose_load(v, i, e)) continue;
            const float chi2 = (float)orbx_pose_error(outlier[i] ? T : Tlast, K, e, pc, err);   // const float chi2 = e->chi2()
            const bool bad = chi2 > (e.stereo ? 7.815f : 5.991f);
            outlier[i] = bad ? 1 : 0;
            if (bad) ++nbad; else ++nactive;
        }
        return nbad;
    }
};
}  // namespace

void orbx_pose_host_run(int nproblems, const orbx_pose_problem *problems, const OrbxPoseCall &c) {
    for (int k = 0; k < nproblems; ++k) {
        const orbx_pose_problem &P = problems[k];
        PoseEvHost ev;
        const int cnt = c.counts[P.frame];
        ev.v.n = cnt < 0 ? 0 : cnt < c.cap ? cnt : c.cap;
        ev.v.kp = c.keys_un + (size_t)P.frame * c.cap;
        ev.v.ur = c.u_right ? c.u_right + (size_t)P.frame * c.cap : nullptr;
        ev.v.pt = c.point + (size_t)k * c.cap;
        ev.v.index = P.point_index;
        ev.v.world = c.world_pos;
        ev.v.sig = c.inv_level_sigma2;
        ev.v.nlevels = c.nlevels;
        ev.v.npoints = P.npoints;
        ev.K.fx = (double)c.camera4[0]; ev.K.fy = (double)c.camera4[1]; ev.K.cx = (double)c.camera4[2]; ev.K.cy = (double)c.camera4[3];
        ev.K.bf = (double)c.mbf;
        ev.outlier = c.outlier + (size_t)k * c.cap;
        int nedges = 0;
        OrbxPoseEdge e;
        if (c.dbg_est) {                                       // the inlier test alone, flags as the caller left them
            for (int i = 0; i < ev.v.n; ++i) nedges += orbx_pose_load(ev.v, i, e) ? 1 : 0;
            c.ninliers[k] = nedges - ev.classify(orbx_pose_from_tcw(c.dbg_est + (size_t)k * 16), orbx_pose_from_tcw(c.dbg_last + (size_t)k * 16));
            continue;
        }
        // Step 3 of the reference: mvbOutlier[i] = false wherever a MapPoint exists, before the early return
        for (int i = 0; i < ev.v.n; ++i)
            if (orbx_pose_load(ev.v, i, e)) { ev.outlier[i] = 0; ++nedges; }
        ev.nactive = nedges;
        if (nedges < 3) { c.ninliers[k] = 0; continue; }       // nInitialCorrespondences < 3: the pose stays as it is
        OrbxPoseSE3 T;
        const int nbad = orbx_pose_rounds(ev, P.Tcw, nedges, &T);
        orbx_pose_to_tcw(T, c.Tcw + (size_t)k * 16);
        c.ninliers[k] = nedges - nbad;
    }
}

extern "C" void orbx_pose_sin_cos(double theta, double *s, double *c) { orbx_pose_sincos(theta, s, c); }
