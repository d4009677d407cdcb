// orbx_map_batches.cpp -- the batched MapPoint refresh, Optimizer::PoseOptimization, the Sim3Solver RANSAC, the PnPsolver RANSAC,
// the Initializer H / F RANSAC and the Initializer's ReconstructH / ReconstructF behind the C ABI: staging, launches and scatter.
// Their HIP-free halves (validation, plans, packing, the host solvers, the Sim3 and PnP cursors, the Initializer results) are
// orbx_mappoint.cpp, orbx_pose.cpp, orbx_sim3.cpp, orbx_pnp.cpp, orbx_init.cpp and orbx_recon.cpp; the three RANSACs go through
// one sequence, ransac_batch_create; the reconstruction has no draws and keeps its own.
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>
#include "orbx_handle.h"

// ---------------------------------------------------------------- MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth,
// batched (orbx_mappoint.h).  One call: validation and plan (orbx_mappoint.cpp), the caller's arrays packed into the page-locked
// block, ONE upload, the launches on the handle's stream, ONE download into the same block, the wait, and the scatter into the
// caller's arrays.
static orbx_status mp_distinct(orbx_handle *h, bool device_form, const uint8_t *d_pool, int64_t pool_rows, int npoints,
                               const int32_t *obs_begin, const uint8_t *desc, const int64_t *obs_row, int32_t *best_idx,
                               int32_t *best_median, uint8_t *best_desc) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    OrbxMpPlan plan;
    const char *why = "";
    orbx_status st = orbx_mp_distinct_plan(npoints, obs_begin, desc, device_form, d_pool, pool_rows, obs_row, best_idx, plan, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    if (npoints == 0) return ORBX_OK;
    if (h->host_only) return orbx_fail(ORBX_NO_DEVICE, "no device handle");
    uint8_t *pin = nullptr, *d = nullptr;
    st = stage_begin(h, std::max(plan.in_bytes, plan.out_bytes), plan.dev_bytes, &pin, &d, false);
    if (st != ORBX_OK) return st;
    if (plan.n_small + plan.n_wide > 0) {
        orbx_mp_distinct_pack(obs_begin, desc, device_form ? obs_row : nullptr, plan, pin);
        st = stage_upload(h, pin, d, plan.in_bytes);
        if (st != ORBX_OK) return st;
        { ProfScope ps(h, ORBX_K_MATCH);
          orbx_launch_mp_distinct(h->stream, (const int32_t *)(d + plan.o_begin), device_form ? d_pool : d + plan.o_rows,
                                  device_form ? (const int64_t *)(d + plan.o_rows) : nullptr, (const int32_t *)(d + plan.o_order),
                                  plan.n_small, plan.n_wide, (int32_t *)(d + plan.o_idx), (int32_t *)(d + plan.o_med),
                                  d + plan.o_desc); }
        st = stage_download_wait(h, pin, d + plan.o_idx, plan.out_bytes);
        if (st != ORBX_OK) return st;
    }
    orbx_mp_distinct_unpack(obs_begin, plan, pin, best_idx, best_median, best_desc);   // (reads no entry of a point without rows)
    return ORBX_OK;
}
extern "C" orbx_status orbx_distinctive_descriptors_batch(orbx_handle *h, int npoints, const int32_t *obs_begin, const uint8_t *desc,
                                                          int32_t *best_idx, int32_t *best_median, uint8_t *best_desc) {
    return mp_distinct(h, false, nullptr, 0, npoints, obs_begin, desc, nullptr, best_idx, best_median, best_desc);
}
extern "C" orbx_status orbx_distinctive_descriptors_batch_device(orbx_handle *h, const uint8_t *d_pool, int64_t pool_rows, int npoints,
                                                                 const int32_t *obs_begin, const int64_t *obs_row, int32_t *best_idx,
                                                                 int32_t *best_median, uint8_t *best_desc) {
    return mp_distinct(h, true, d_pool, pool_rows, npoints, obs_begin, nullptr, obs_row, best_idx, best_median, best_desc);
}
extern "C" orbx_status orbx_update_normal_and_depth_batch(orbx_handle *h, int npoints, const int32_t *obs_begin, const float *pos,
                                                          const float *centers, const float *ref_center, const int32_t *ref_level,
                                                          float *normal, float *min_distance, float *max_distance) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    OrbxMpNormalPlan plan;
    const char *why = "";
    orbx_status st = orbx_mp_normal_plan(npoints, obs_begin, pos, centers, ref_center, ref_level, h->p.nlevels, normal, min_distance,
                                         max_distance, plan, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    if (npoints == 0) return ORBX_OK;
    if (h->host_only) return orbx_fail(ORBX_NO_DEVICE, "no device handle");
    if (plan.nrows == 0) return ORBX_OK;                             // no point has rows: nothing is written
    uint8_t *pin = nullptr, *d = nullptr;
    st = stage_begin(h, std::max(plan.in_bytes, plan.out_bytes), plan.dev_bytes, &pin, &d, false);
    if (st != ORBX_OK) return st;
    orbx_mp_normal_pack(obs_begin, pos, centers, ref_center, ref_level, h->tab.scale, plan, pin);
    st = stage_upload(h, pin, d, plan.in_bytes);
    if (st != ORBX_OK) return st;
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_mp_normal_depth(h->stream, (const int32_t *)(d + plan.o_begin), (const DMpPoint *)(d + plan.o_points),
                                  (const float *)(d + plan.o_centers), npoints, h->tab.scale[h->p.nlevels - 1],
                                  (float *)(d + plan.o_out)); }
    st = stage_download_wait(h, pin, d + plan.o_out, plan.out_bytes);
    if (st != ORBX_OK) return st;
    orbx_mp_normal_unpack(obs_begin, plan, pin, normal, min_distance, max_distance);
    return ORBX_OK;
}

// ---------------------------------------------------------------- Optimizer::PoseOptimization(Frame*), batched (orbx_pose.h).
// Device path: validation and layout (orbx_pose.cpp), all problems' host state and the pool packed into the page-locked
// block, ONE upload, k_pose_opt on the handle's stream; nothing downloaded, nothing waited for.  Host path
// (ORBX_POSE=host, read per call; host-only handles, where the "d_" arguments are host arrays): the same header compiled by
// the host compiler.  On a device handle it downloads the rows it needs, runs, and uploads the results -- a cross-check, not a
// fast path.
static bool host_selected(const char *var) {                  // ORBX_POSE / ORBX_SIM3 / ORBX_PNP / ORBX_INIT / ORBX_RECON / ORBX_LOCALBA = host, read per call
    const char *e = getenv(var);
    return e && strcmp(e, "host") == 0;
}
static orbx_status pose_batch(orbx_handle *h, int nproblems, const orbx_pose_problem *problems, int npool, const float *world_pos,
                              int nframes, const orbx_keypoint *d_keys_un, const float *d_u_right, const int32_t *d_counts, int cap,
                              const int32_t *d_point, const float *camera4, float mbf, const float *inv_level_sigma2, int nlevels,
                              float *d_Tcw, uint8_t *d_outlier, int32_t *d_ninliers, const float *dbg_est, const float *dbg_last) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    OrbxPoseCall c;
    c.npool = npool; c.nframes = nframes; c.cap = cap; c.nlevels = nlevels;
    c.world_pos = world_pos; c.camera4 = camera4; c.inv_level_sigma2 = inv_level_sigma2; c.mbf = mbf;
    c.keys_un = d_keys_un; c.u_right = d_u_right; c.counts = d_counts; c.point = d_point;
    c.Tcw = d_Tcw; c.outlier = d_outlier; c.ninliers = d_ninliers; c.dbg_est = dbg_est; c.dbg_last = dbg_last;
    OrbxPosePlan plan;
    const char *why = "";
    orbx_status st = orbx_pose_plan(nproblems, problems, c, plan, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    if (nproblems == 0) return ORBX_OK;
    if (h->host_only) {
        st = orbx_pose_check_rows(nproblems, problems, c, &why);
        if (st != ORBX_OK) return orbx_fail(st, why);
        orbx_pose_host_run(nproblems, problems, c);
        return ORBX_OK;
    }
    if (host_selected("ORBX_POSE")) {
        HIPCHK(hipSetDevice(h->dev));
        const size_t fr = (size_t)nframes * cap, pr = (size_t)nproblems * cap;
        std::vector<orbx_keypoint> keys(fr);
        std::vector<float> ur(d_u_right ? fr : 0), T((size_t)nproblems * 16);
        std::vector<int32_t> counts((size_t)nframes), point(pr), nin((size_t)nproblems);
        std::vector<uint8_t> outl(pr);
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(keys.data(), d_keys_un, fr * sizeof(orbx_keypoint), hipMemcpyDeviceToHost));
        if (d_u_right) HIPCHK(hipMemcpy(ur.data(), d_u_right, fr * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(counts.data(), d_counts, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(point.data(), d_point, pr * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(outl.data(), d_outlier, pr, hipMemcpyDeviceToHost));
        if (!dbg_est) HIPCHK(hipMemcpy(T.data(), d_Tcw, T.size() * sizeof(float), hipMemcpyDeviceToHost));
        // the kernel's rule for what the host cannot validate on device rows: such a feature has no MapPoint (orbx_pose_load)
        c.keys_un = keys.data(); c.u_right = d_u_right ? ur.data() : nullptr; c.counts = counts.data(); c.point = point.data();
        c.Tcw = T.data(); c.outlier = outl.data(); c.ninliers = nin.data();
        orbx_pose_host_run(nproblems, problems, c);
        HIPCHK(hipMemcpy(d_outlier, outl.data(), pr, hipMemcpyHostToDevice));
        if (!dbg_est) HIPCHK(hipMemcpy(d_Tcw, T.data(), T.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_ninliers, nin.data(), nin.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        return ORBX_OK;
    }
    uint8_t *pin = nullptr, *d = nullptr;
    st = stage_begin(h, plan.in_bytes, plan.in_bytes, &pin, &d, true);
    if (st != ORBX_OK) return st;
    orbx_pose_pack(problems, c, plan, pin);
    st = stage_upload(h, pin, d, plan.in_bytes);
    if (st != ORBX_OK) return st;
    DPoseArgs a;
    a.prob = (const DPoseProb *)(d + plan.o_prob);
    a.index = (const int32_t *)(d + plan.o_index);
    a.world = (const float *)(d + plan.o_world);
    a.sig = (const float *)(d + plan.o_sig);
    a.kps = d_keys_un; a.ur = d_u_right; a.counts = d_counts; a.point = d_point;
    a.cap = cap; a.nlevels = nlevels; a.nproblems = nproblems;
    a.fx = camera4[0]; a.fy = camera4[1]; a.cx = camera4[2]; a.cy = camera4[3]; a.mbf = mbf;
    a.Tcw = d_Tcw; a.outlier = d_outlier; a.ninliers = d_ninliers;
    a.dbg = dbg_est ? (const float *)(d + plan.o_dbg) : nullptr;
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_pose_opt(h->stream, a); }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    return ORBX_OK;
}
extern "C" orbx_status orbx_pose_optimization_batch_device(orbx_handle *h, int nproblems, const orbx_pose_problem *problems, int npool,
                                                           const float *world_pos, int nframes, const orbx_keypoint *d_keys_un,
                                                           const float *d_u_right, const int32_t *d_counts, int cap,
                                                           const int32_t *d_point, const float *camera4, float mbf,
                                                           const float *inv_level_sigma2, int nlevels, float *d_Tcw,
                                                           uint8_t *d_outlier, int32_t *d_ninliers) {
    return pose_batch(h, nproblems, problems, npool, world_pos, nframes, d_keys_un, d_u_right, d_counts, cap, d_point, camera4, mbf,
                      inv_level_sigma2, nlevels, d_Tcw, d_outlier, d_ninliers, nullptr, nullptr);
}
extern "C" orbx_status orbx_debug_pose_inlier_test(orbx_handle *h, int nproblems, const orbx_pose_problem *problems, int npool,
                                                   const float *world_pos, int nframes, const orbx_keypoint *d_keys_un,
                                                   const float *d_u_right, const int32_t *d_counts, int cap, const int32_t *d_point,
                                                   const float *camera4, float mbf, const float *inv_level_sigma2, int nlevels,
                                                   const float *Tcw_est, const float *Tcw_last, uint8_t *d_outlier,
                                                   int32_t *d_ninliers) {
    if (!Tcw_est || !Tcw_last) return orbx_fail(ORBX_BAD_ARGUMENT, "null pose array");
    float unused[16];   // the pose rows are not written by the inlier test; the plan only wants a non-null pointer
    return pose_batch(h, nproblems, problems, npool, world_pos, nframes, d_keys_un, d_u_right, d_counts, cap, d_point, camera4, mbf,
                      inv_level_sigma2, nlevels, unused, d_outlier, d_ninliers, Tcw_est, Tcw_last);
}
extern "C" orbx_status orbx_pose_optimization(orbx_handle *h, float *Tcw, int n, const orbx_keypoint *keys_un, const float *u_right,
                                              const int32_t *point, int npool, const float *world_pos, const float *camera4,
                                              float mbf, const float *inv_level_sigma2, int nlevels, uint8_t *outlier,
                                              int32_t *ninliers) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    if (!Tcw || n <= 0) return orbx_fail(ORBX_BAD_ARGUMENT, !Tcw ? "null Tcw" : "n <= 0");
    orbx_pose_problem P;
    P.frame = 0; P.point_index = nullptr; P.npoints = npool;
    memcpy(P.Tcw, Tcw, sizeof(P.Tcw));
    const int32_t count = n;
    OrbxPoseCall c;
    c.npool = npool; c.nframes = 1; c.cap = n; c.nlevels = nlevels; c.batch_form = false;
    c.world_pos = world_pos; c.camera4 = camera4; c.inv_level_sigma2 = inv_level_sigma2; c.mbf = mbf;
    c.keys_un = keys_un; c.u_right = u_right; c.counts = &count; c.point = point;
    c.Tcw = Tcw; c.outlier = outlier; c.ninliers = ninliers;
    OrbxPosePlan plan;
    const char *why = "";
    orbx_status st = orbx_pose_plan(1, &P, c, plan, &why);
    if (st == ORBX_OK) st = orbx_pose_check_rows(1, &P, c, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    orbx_pose_host_run(1, &P, c);
    return ORBX_OK;
}

// ---------------------------------------------------------------- Optimizer::OptimizeSim3, batched (orbx_sim3opt.h).
// Device path: validation and layout (orbx_sim3opt.cpp), all problems packed into the page-locked block, ONE upload, k_sim3_opt
// on the handle's stream, ONE download of results | keep, the wait, the scatter.  Host path (ORBX_SIM3OPT=host, read per call;
// host-only handles): the same header compiled by the host compiler over the same packed block.
static orbx_status sim3opt_batch(orbx_handle *h, int nproblems, const orbx_sim3opt_problem *problems, const double *last,
                                 bool inlier_test, orbx_sim3opt_result *results) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    OrbxSim3OptPlan plan;
    const char *why = "";
    orbx_status st = orbx_sim3opt_plan(nproblems, problems, results, last, inlier_test, plan, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    if (nproblems == 0) return ORBX_OK;
    if (h->host_only || host_selected("ORBX_SIM3OPT")) {
        std::vector<uint8_t> in(plan.in_bytes), out(plan.out_bytes);
        orbx_sim3opt_pack(problems, last, plan, in.data());
        orbx_sim3opt_host_run(plan, in.data(), inlier_test, out.data());
        orbx_sim3opt_unpack(problems, plan, out.data(), results);
        return ORBX_OK;
    }
    uint8_t *pin = nullptr, *d = nullptr;
    const size_t dev_in = pad256(plan.in_bytes);
    st = stage_begin(h, std::max(plan.in_bytes, plan.out_bytes), dev_in + plan.out_bytes, &pin, &d, false);
    if (st != ORBX_OK) return st;
    orbx_sim3opt_pack(problems, last, plan, pin);
    st = stage_upload(h, pin, d, plan.in_bytes);
    if (st != ORBX_OK) return st;
    DSim3OptArgs a;
    a.prob = (const DSim3OptProb *)(d + plan.o_prob);
    a.pts = (const float *)(d + plan.o_pts);
    a.res = (orbx_sim3opt_result *)(d + dev_in + plan.o_res);
    a.keep = d + dev_in + plan.o_keep;
    a.nproblems = nproblems; a.inlier_test_only = inlier_test ? 1 : 0;
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_sim3_opt(h->stream, a); }
    st = stage_download_wait(h, pin, d + dev_in, plan.out_bytes);
    if (st != ORBX_OK) return st;
    orbx_sim3opt_unpack(problems, plan, pin, results);
    return ORBX_OK;
}
extern "C" orbx_status orbx_optimize_sim3_batch(orbx_handle *h, int nproblems, const orbx_sim3opt_problem *problems,
                                                orbx_sim3opt_result *results) {
    return sim3opt_batch(h, nproblems, problems, nullptr, false, results);
}
extern "C" orbx_status orbx_debug_sim3opt_inlier_test(orbx_handle *h, int nproblems, const orbx_sim3opt_problem *problems,
                                                      const double *S_last, orbx_sim3opt_result *results) {
    return sim3opt_batch(h, nproblems, problems, S_last, true, results);
}

// ---------------------------------------------------------------- Optimizer::LocalBundleAdjustment, batched (orbx_localba.h).
// Device path: validation, layout and the derived index lists (orbx_localba.cpp), all problems packed into the page-locked block,
// ONE upload, k_local_ba on the handle's stream, ONE download of results | poses | points | erase, the wait, the scatter.  The
// device block is input | workspace | output.  Host path (ORBX_LOCALBA=host, read per call; host-only handles): the same header
// compiled by the host compiler over the same packed block.
static orbx_status localba_batch(orbx_handle *h, int nproblems, const orbx_localba_problem *problems, const orbx_localba_debug *dbg,
                                 bool debug, orbx_localba_result *results) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    OrbxLbaPlan plan;
    std::vector<DLbaProb> probs;
    const char *why = "";
    orbx_status st = orbx_localba_plan(nproblems, problems, results, dbg, debug, plan, probs, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    if (nproblems == 0) return ORBX_OK;
    if (h->host_only || host_selected("ORBX_LOCALBA")) {
        std::vector<uint8_t> in(plan.in_bytes), work(plan.work_bytes), out(plan.out_bytes);
        orbx_localba_pack(problems, dbg, plan, probs, in.data());
        orbx_localba_host_run(plan, in.data(), work.data(), out.data());
        orbx_localba_unpack(problems, probs, out.data(), debug, results);
        return ORBX_OK;
    }
    uint8_t *pin = nullptr, *d = nullptr;
    const size_t dev_in = pad256(plan.in_bytes), dev_work = pad256(plan.work_bytes);
    st = stage_begin(h, std::max(plan.in_bytes, plan.out_bytes), dev_in + dev_work + plan.out_bytes, &pin, &d, false);
    if (st != ORBX_OK) return st;
    orbx_localba_pack(problems, dbg, plan, probs, pin);
    st = stage_upload(h, pin, d, plan.in_bytes);
    if (st != ORBX_OK) return st;
    DLbaArgs a;
    a.prob = (const DLbaProb *)(d + plan.o_prob);
    a.in = d; a.work = d + dev_in; a.out = d + dev_in + dev_work;
    a.nproblems = nproblems;
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_local_ba(h->stream, a); }
    st = stage_download_wait(h, pin, a.out, plan.out_bytes);
    if (st != ORBX_OK) return st;
    orbx_localba_unpack(problems, probs, pin, debug, results);
    return ORBX_OK;
}
extern "C" orbx_status orbx_local_bundle_adjustment_batch(orbx_handle *h, int nproblems, const orbx_localba_problem *problems,
                                                          orbx_localba_result *results) {
    return localba_batch(h, nproblems, problems, nullptr, false, results);
}
extern "C" orbx_status orbx_debug_localba_classify(orbx_handle *h, int nproblems, const orbx_localba_problem *problems,
                                                   const orbx_localba_debug *states, orbx_localba_result *results) {
    return localba_batch(h, nproblems, problems, states, true, results);
}

// ---------------------------------------------------------------- Optimizer::OptimizeEssentialGraph, batched (orbx_essgraph.h).
// Device path: validation, the elimination order and the symbolic factorisation (orbx_essgraph.cpp; a problem above
// ORBX_EG_MAX_LBLOCKS is ORBX_CAPACITY here), all problems packed into the page-locked block, ONE upload, k_essential_graph and
// k_eg_correct_points on the handle's stream, ONE download of results | Siw | Tiw | points, the wait, the scatter.  The device
// block is input | workspace | output.  Host path (ORBX_ESSGRAPH=host, read per call; host-only handles): the same header
// compiled by the host compiler over the same packed block, without the cap.
extern "C" orbx_status orbx_optimize_essential_graph_batch(orbx_handle *h, int nproblems, const orbx_essgraph_problem *problems,
                                                           orbx_essgraph_result *results) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    const bool host = h->host_only || host_selected("ORBX_ESSGRAPH");
    OrbxEgPlan plan;
    const char *why = "";
    orbx_status st = orbx_eg_plan(nproblems, problems, results, !host, plan, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    if (nproblems == 0) return ORBX_OK;
    if (host) {
        std::vector<uint8_t> in(plan.in_bytes), work(plan.work_bytes), out(plan.out_bytes);
        orbx_eg_pack(problems, plan, in.data());
        orbx_eg_host_run(plan, in.data(), work.data(), out.data());
        orbx_eg_unpack(problems, plan, out.data(), results);
        return ORBX_OK;
    }
    uint8_t *pin = nullptr, *d = nullptr;
    const size_t dev_in = pad256(plan.in_bytes), dev_work = pad256(plan.work_bytes);
    st = stage_begin(h, std::max(plan.in_bytes, plan.out_bytes), dev_in + dev_work + plan.out_bytes, &pin, &d, false);
    if (st != ORBX_OK) return st;
    orbx_eg_pack(problems, plan, pin);
    st = stage_upload(h, pin, d, plan.in_bytes);
    if (st != ORBX_OK) return st;
    DEgArgs a;
    a.prob = (const DEgProb *)(d + plan.o_prob);
    a.in = d; a.work = d + dev_in; a.out = d + dev_in + dev_work;
    a.nproblems = nproblems;
    a.npoints = plan.npoints; a.o_pts_in = (int64_t)plan.o_pts_in; a.o_pts_out = (int64_t)plan.o_pts_out;
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_essential_graph(h->stream, a); }
    st = stage_download_wait(h, pin, a.out, plan.out_bytes);
    if (st != ORBX_OK) return st;
    orbx_eg_unpack(problems, plan, pin, results);
    return ORBX_OK;
}

// ---------------------------------------------------------------- the batched RANSACs (orbx_ransac.h): one sequence for all.
// Device path: validation and layout (S::plan), all problems packed into the page-locked block, ONE upload, the solver's two
// kernels on the handle's stream (S::launch), ONE download of hypotheses | masks | tally, the wait; the batch keeps a host copy
// (S::batch_take) and every later call reads that.  Host path (S::env = host, read per call; host-only handles): the same
// header compiled by the host compiler over the same packed block (S::host_run).  S::keeps_block: the batch keeps the result
// block as it is (batch->out, allocated by S::batch_new), so the host path runs straight into it.
template <class S>
static orbx_status ransac_batch_create(orbx_handle *h, int nproblems, const typename S::problem *problems, typename S::batch **out) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    if (!out) return orbx_fail(ORBX_BAD_ARGUMENT, "null batch pointer");
    OrbxRansacPlan plan;
    const char *why = "";
    orbx_status st = S::plan(nproblems, problems, plan, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    if (plan.nlaunch == 0) {                                   // nothing to compute: the batch says so for every problem
        *out = S::batch_new(problems, plan);
        return ORBX_OK;
    }
    if (h->host_only || host_selected(S::env)) {
        std::vector<uint8_t> in(plan.in_bytes), res(S::keeps_block ? 0 : plan.out_bytes);
        S::pack(problems, plan, in.data());
        typename S::batch *b = *out = S::batch_new(problems, plan);
        if constexpr (S::keeps_block) S::host_run(plan, in.data(), b->out.data());   // straight into the batch's block: nothing to take
        else { S::host_run(plan, in.data(), res.data()); S::batch_take(b, plan, res.data()); }
        return ORBX_OK;
    }
    uint8_t *pin = nullptr, *d = nullptr;
    const size_t dev_in = pad256(plan.in_bytes);
    st = stage_begin(h, std::max(plan.in_bytes, plan.out_bytes), dev_in + plan.out_bytes, &pin, &d, false);
    if (st != ORBX_OK) return st;
    S::pack(problems, plan, pin);
    st = stage_upload(h, pin, d, plan.in_bytes);
    if (st != ORBX_OK) return st;
    { ProfScope ps(h, ORBX_K_MISC);
      S::launch(h->stream, orbx_ransac_args<typename S::args>(plan, d, d + dev_in)); }
    st = stage_download_wait(h, pin, d + dev_in, plan.out_bytes);
    if (st != ORBX_OK) return st;
    *out = S::batch_new(problems, plan);
    S::batch_take(*out, plan, pin);
    return ORBX_OK;
}
// fail_why(f(..., &why), why): `why` is taken by reference, so it is read here, after f has set it, whichever argument the
// compiler evaluates first
static orbx_status fail_why(orbx_status st, const char *const &why) { return st == ORBX_OK ? st : orbx_fail(st, why); }

// ---------------------------------------------------------------- Sim3Solver RANSAC, batched (orbx_sim3.h): k_sim3_hypotheses and
// k_sim3_inliers; the batch keeps the downloaded block as it is and iterate() is a cursor over it.
struct Sim3Frame {
    using problem = orbx_sim3_problem; using batch = orbx_sim3_batch; using args = DSim3Args;
    static constexpr const char *env = "ORBX_SIM3"; static constexpr bool keeps_block = true;
    static constexpr auto plan = orbx_sim3_plan; static constexpr auto pack = orbx_sim3_pack;
    static constexpr auto host_run = orbx_sim3_host_run; static constexpr auto launch = orbx_launch_sim3;
    static constexpr auto batch_new = orbx_sim3_batch_new; static constexpr auto batch_take = orbx_sim3_batch_take;
};
extern "C" orbx_status orbx_sim3_ransac_batch_create(orbx_handle *h, int nproblems, const orbx_sim3_problem *problems,
                                                     orbx_sim3_batch **out) {
    return ransac_batch_create<Sim3Frame>(h, nproblems, problems, out);
}
extern "C" int32_t orbx_sim3_batch_iterate(orbx_sim3_batch *b, int k, int n_iterations, int32_t *no_more, uint8_t *inliers,
                                           int32_t *ninliers, float *T12) {
    const char *why = "";
    const int32_t r = orbx_sim3_cursor_iterate(b, k, n_iterations, no_more, inliers, ninliers, T12, &why);
    if (r < 0) orbx_fail(ORBX_BAD_ARGUMENT, why);
    return r;
}
extern "C" orbx_status orbx_sim3_batch_best(const orbx_sim3_batch *b, int k, float *R, float *t, float *s) {
    const char *why = "";
    return fail_why(orbx_sim3_cursor_best(b, k, R, t, s, &why), why);
}
extern "C" orbx_status orbx_sim3_batch_counts(const orbx_sim3_batch *b, int k, int32_t *counts, int32_t *niterations) {
    const char *why = "";
    return fail_why(orbx_sim3_cursor_counts(b, k, counts, niterations, &why), why);
}
extern "C" orbx_status orbx_sim3_batch_hypothesis(const orbx_sim3_batch *b, int k, int iteration, float *hyp48, uint64_t *mask_words) {
    const char *why = "";
    return fail_why(orbx_sim3_cursor_hypothesis(b, k, iteration, hyp48, mask_words, &why), why);
}
extern "C" void orbx_sim3_batch_destroy(orbx_sim3_batch *b) { delete b; }

// ---------------------------------------------------------------- PnPsolver RANSAC, batched (orbx_pnp.h): k_pnp_hypotheses and
// k_pnp_inliers; the batch keeps the results per solver (append() adds to them) and iterate() is a cursor over them.
struct PnpFrame {
    using problem = orbx_pnp_problem; using batch = orbx_pnp_batch; using args = DPnpArgs;
    static constexpr const char *env = "ORBX_PNP"; static constexpr bool keeps_block = false;
    static constexpr auto plan = orbx_pnp_plan; static constexpr auto pack = orbx_pnp_pack;
    static constexpr auto host_run = orbx_pnp_host_run; static constexpr auto launch = orbx_launch_pnp;
    static constexpr auto batch_new = orbx_pnp_batch_new; static constexpr auto batch_take = orbx_pnp_batch_take;
};
extern "C" orbx_status orbx_pnp_ransac_batch_create(orbx_handle *h, int nproblems, const orbx_pnp_problem *problems,
                                                    orbx_pnp_batch **out) {
    return ransac_batch_create<PnpFrame>(h, nproblems, problems, out);
}
extern "C" int32_t orbx_pnp_batch_iterate(orbx_pnp_batch *b, int k, int n_iterations, int32_t *no_more, uint8_t *inliers,
                                          int32_t *ninliers, float *Tcw) {
    const char *why = "";
    const int32_t r = orbx_pnp_cursor_iterate(b, k, n_iterations, no_more, inliers, ninliers, Tcw, &why);
    if (r < 0) orbx_fail(ORBX_BAD_ARGUMENT, why);             // -2 (append sets and call again) records its message too
    return r;
}
extern "C" orbx_status orbx_pnp_batch_append(orbx_pnp_batch *b, int k, int nsets, const int32_t *sets) {
    const char *why = "";
    return fail_why(orbx_pnp_cursor_append(b, k, nsets, sets, &why), why);
}
extern "C" orbx_status orbx_pnp_batch_best(const orbx_pnp_batch *b, int k, float *Tcw, int32_t *ninliers, int32_t *iteration) {
    const char *why = "";
    return fail_why(orbx_pnp_cursor_best(b, k, Tcw, ninliers, iteration, &why), why);
}
extern "C" orbx_status orbx_pnp_batch_counts(const orbx_pnp_batch *b, int k, int32_t *counts, int32_t *niterations) {
    const char *why = "";
    return fail_why(orbx_pnp_cursor_counts(b, k, counts, niterations, &why), why);
}
extern "C" orbx_status orbx_pnp_batch_hypothesis(const orbx_pnp_batch *b, int k, int iteration, double *Rt12, float *Tcw, int32_t *N,
                                                 uint64_t *mask_words) {
    const char *why = "";
    return fail_why(orbx_pnp_cursor_hypothesis(b, k, iteration, Rt12, Tcw, N, mask_words, &why), why);
}
extern "C" void orbx_pnp_batch_destroy(orbx_pnp_batch *b) { delete b; }

// ---------------------------------------------------------------- Initializer H / F RANSAC, batched (orbx_init.h):
// k_init_hypotheses and k_init_scores; the batch keeps the results per problem and picks the best iteration of each model on the
// host (orbx_init_batch_take).  A problem that computes nothing reports ORBX_INIT_NONE.
struct InitFrame {
    using problem = orbx_init_problem; using batch = orbx_init_batch; using args = DInitArgs;
    static constexpr const char *env = "ORBX_INIT"; static constexpr bool keeps_block = false;
    static constexpr auto plan = orbx_init_plan; static constexpr auto pack = orbx_init_pack;
    static constexpr auto host_run = orbx_init_host_run; static constexpr auto launch = orbx_launch_init;
    static constexpr auto batch_new = orbx_init_batch_new; static constexpr auto batch_take = orbx_init_batch_take;
};
extern "C" orbx_status orbx_init_ransac_batch_create(orbx_handle *h, int nproblems, const orbx_init_problem *problems,
                                                     orbx_init_batch **out) {
    return ransac_batch_create<InitFrame>(h, nproblems, problems, out);
}
extern "C" orbx_status orbx_init_batch_result(const orbx_init_batch *b, int k, float *SH, float *SF, float *H21, float *F21,
                                              uint8_t *inliersH, uint8_t *inliersF, int32_t *itH, int32_t *itF, float *RH,
                                              int32_t *model) {
    const char *why = "";
    return fail_why(orbx_init_get_result(b, k, SH, SF, H21, F21, inliersH, inliersF, itH, itF, RH, model, &why), why);
}
extern "C" orbx_status orbx_init_batch_scores(const orbx_init_batch *b, int k, int model, float *scores, int32_t *niterations) {
    const char *why = "";
    return fail_why(orbx_init_get_scores(b, k, model, scores, niterations, &why), why);
}
extern "C" orbx_status orbx_init_batch_hypothesis(const orbx_init_batch *b, int k, int model, int iteration, float *M9, float *Minv9,
                                                  float *score, uint64_t *mask_words) {
    const char *why = "";
    return fail_why(orbx_init_get_hypothesis(b, k, model, iteration, M9, Minv9, score, mask_words, &why), why);
}
extern "C" orbx_status orbx_init_batch_normalization(const orbx_init_batch *b, int k, float *T1, float *T2) {
    const char *why = "";
    return fail_why(orbx_init_get_normalization(b, k, T1, T2, &why), why);
}
extern "C" void orbx_init_batch_destroy(orbx_init_batch *b) { delete b; }

// ---------------------------------------------------------------- Initializer ReconstructH / ReconstructF, batched (orbx_recon.h):
// k_init_decompose, k_init_check_rt and k_init_pick; the batch keeps the results per problem and runs acos and the accept / reject
// arithmetic on the host (orbx_recon_batch_take).  Not the RANSAC frame: this batch has no draws, no sets and no groups.
// Device block: uploaded | downloaded | work (the per-hypothesis planes, never downloaded).
extern "C" orbx_status orbx_init_reconstruct_batch_create(orbx_handle *h, int nproblems, const orbx_recon_problem *problems,
                                                          orbx_recon_batch **out) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    if (!out) return orbx_fail(ORBX_BAD_ARGUMENT, "null batch pointer");
    OrbxReconPlan plan;
    const char *why = "";
    orbx_status st = orbx_recon_plan(nproblems, problems, plan, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    if (plan.nlaunch == 0) {                                   // nothing to compute: the batch says so for every problem
        *out = orbx_recon_batch_new(problems, plan);
        return ORBX_OK;
    }
    if (h->host_only || host_selected("ORBX_RECON")) {
        std::vector<uint8_t> in(plan.in_bytes), res(plan.out_bytes);
        orbx_recon_pack(problems, plan, in.data());
        orbx_recon_host_run(plan, in.data(), res.data());
        *out = orbx_recon_batch_new(problems, plan);
        orbx_recon_batch_take(*out, plan, res.data());
        return ORBX_OK;
    }
    uint8_t *pin = nullptr, *d = nullptr;
    st = stage_begin(h, std::max(plan.in_bytes, plan.out_bytes), plan.in_bytes + plan.out_bytes + plan.work_bytes, &pin, &d, false);
    if (st != ORBX_OK) return st;
    orbx_recon_pack(problems, plan, pin);
    st = stage_upload(h, pin, d, plan.in_bytes);
    if (st != ORBX_OK) return st;
    uint8_t *d_out = d + plan.in_bytes;
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_recon(h->stream, orbx_recon_args(plan, d, d_out + plan.out_bytes, d_out, nullptr)); }
    st = stage_download_wait(h, pin, d_out, plan.out_bytes);
    if (st != ORBX_OK) return st;
    *out = orbx_recon_batch_new(problems, plan);
    orbx_recon_batch_take(*out, plan, pin);
    return ORBX_OK;
}
extern "C" orbx_status orbx_recon_batch_result(const orbx_recon_batch *b, int k, int32_t *ok, float *R21, float *t21, int32_t *chosen,
                                               uint8_t *status, float *points, int32_t *N) {
    const char *why = "";
    return fail_why(orbx_recon_get_result(b, k, ok, R21, t21, chosen, status, points, N, &why), why);
}
extern "C" orbx_status orbx_recon_batch_hypothesis(const orbx_recon_batch *b, int k, int i, float *R9, float *t3, float *n3,
                                                   int32_t *nGood, float *cosine, float *parallax, int32_t *valid) {
    const char *why = "";
    return fail_why(orbx_recon_get_hypothesis(b, k, i, R9, t3, n3, nGood, cosine, parallax, valid, &why), why);
}
extern "C" void orbx_recon_batch_destroy(orbx_recon_batch *b) { delete b; }

// Initializer::Initialize from :204 to its return.  Fused: the RANSAC's block and the reconstruction's records go up in one copy,
// k_init_hypotheses, k_init_scores, k_init_select, k_init_decompose, k_init_check_rt, k_init_pick run on the handle's stream, the
// RANSAC's results and the reconstruction's come down in one copy.  Device block: RANSAC in | records | RANSAC out | recon out |
// work.  With a host switch set, or on a host-only handle: the two calls, one after the other.
extern "C" orbx_status orbx_initialize_batch_create(orbx_handle *h, int nproblems, const orbx_init_problem *problems,
                                                    const orbx_init_camera *cameras, orbx_init_batch **ransac,
                                                    orbx_recon_batch **recon) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    if (!ransac || !recon) return orbx_fail(ORBX_BAD_ARGUMENT, "null batch pointer");
    OrbxInitPlan ip;
    OrbxReconPlan rp;
    const char *why = "";
    orbx_status st = orbx_init_plan(nproblems, problems, ip, &why);
    if (st == ORBX_OK) st = orbx_recon_fused_plan(nproblems, problems, cameras, rp, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    if (ip.nlaunch == 0 || h->host_only || host_selected("ORBX_INIT") || host_selected("ORBX_RECON")) {
        st = orbx_init_ransac_batch_create(h, nproblems, problems, ransac);
        if (st != ORBX_OK) return st;
        std::vector<orbx_recon_problem> rprob;
        std::vector<std::vector<uint8_t>> store;
        orbx_recon_problems_from(problems, cameras, *ransac, rprob, store);
        st = orbx_init_reconstruct_batch_create(h, nproblems, rprob.data(), recon);
        if (st != ORBX_OK) { delete *ransac; *ransac = nullptr; }
        return st;
    }
    const size_t init_in = pad256(ip.in_bytes), init_out = pad256(ip.out_bytes);
    const size_t in_total = init_in + rp.in_bytes, out_total = init_out + rp.out_bytes;
    uint8_t *pin = nullptr, *d = nullptr;
    st = stage_begin(h, std::max(in_total, out_total), in_total + out_total + rp.work_bytes, &pin, &d, false);
    if (st != ORBX_OK) return st;
    orbx_init_pack(problems, ip, pin);
    orbx_recon_fused_pack(problems, cameras, rp, pin + init_in);
    st = stage_upload(h, pin, d, in_total);
    if (st != ORBX_OK) return st;
    uint8_t *d_out = d + in_total;
    { ProfScope ps(h, ORBX_K_MISC);
      const DInitArgs ia = orbx_ransac_args<DInitArgs>(ip, d, d_out);
      const DReconArgs ra = orbx_recon_args(rp, d + init_in, d_out + out_total, d_out + init_out, ia.pts);
      orbx_launch_init(h->stream, ia);
      orbx_launch_init_select(h->stream, ia, ra);
      orbx_launch_recon(h->stream, ra); }
    st = stage_download_wait(h, pin, d_out, out_total);
    if (st != ORBX_OK) return st;
    *ransac = orbx_init_batch_new(problems, ip);
    orbx_init_batch_take(*ransac, ip, pin);
    *recon = orbx_recon_batch_new_fused(cameras, *ransac);
    orbx_recon_batch_take(*recon, rp, pin + init_out);
    return ORBX_OK;
}

// ---------------------------------------------------------------- LocalMapping::CreateNewMapPoints, the per-match geometry,
// batched (orbx_newpoints.h).  Device path: validation and layout (orbx_newpoints.cpp), the cameras, the chunk table and the
// operands gathered by index packed into the page-locked block, ONE upload, k_new_points on the handle's stream, ONE download of
// status | points, the wait, the scatter.  Host path (ORBX_NEWPOINTS=host, read per call; host-only handles): the same header
// compiled by the host compiler over the same packed block.
extern "C" orbx_status orbx_create_new_map_points_batch(orbx_handle *h, int nproblems, const orbx_newpoints_problem *problems,
                                                        uint8_t *status_out, float *points_out) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    OrbxNewPtsPlan plan;
    const char *why = "";
    orbx_status st = orbx_newpoints_plan(nproblems, problems, status_out, points_out, plan, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    if (plan.total == 0) return ORBX_OK;                         // no problem, or none with a match: nothing launches
    if (h->host_only || host_selected("ORBX_NEWPOINTS")) {
        std::vector<uint8_t> in(plan.in_bytes), out(plan.out_bytes);
        orbx_newpoints_pack(problems, plan, in.data());
        orbx_newpoints_host_run(plan, in.data(), out.data());
        orbx_newpoints_unpack(plan, out.data(), status_out, points_out);
        return ORBX_OK;
    }
    uint8_t *pin = nullptr, *d = nullptr;
    const size_t dev_in = pad256(plan.in_bytes);
    st = stage_begin(h, std::max(plan.in_bytes, plan.out_bytes), dev_in + plan.out_bytes, &pin, &d, false);
    if (st != ORBX_OK) return st;
    orbx_newpoints_pack(problems, plan, pin);
    st = stage_upload(h, pin, d, plan.in_bytes);
    if (st != ORBX_OK) return st;
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_new_points(h->stream, orbx_newpoints_args(plan, d, d + dev_in)); }
    st = stage_download_wait(h, pin, d + dev_in, plan.out_bytes);
    if (st != ORBX_OK) return st;
    orbx_newpoints_unpack(plan, pin, status_out, points_out);
    return ORBX_OK;
}

// ---------------------------------------------------------------- ORBmatcher::SearchBySim3, batched, pose algebra included
// (orbx_sim3search.h).  Device path: validation and layout (orbx_sim3search.cpp), the keyframe pool -- each keyframe once -- and
// the problems packed into the page-locked block, ONE upload, k_grid_build over the pool + k_sim3s_project + k_sim3s_cand +
// k_sim3s_mutual on the handle's stream, ONE download (counts | matches, and the debug rows where asked for), the wait, the
// scatter.  Host path (ORBX_SIM3SEARCH=host, read per call; host-only handles): the same header over the same packed block.
extern "C" orbx_status orbx_search_by_sim3_batch(orbx_handle *h, int nkeyframes, const orbx_sim3_search_keyframe *keyframes,
                                                 int nproblems, const orbx_sim3_search_problem *problems, const float *camera4,
                                                 const float *bounds4, int32_t *const *matches12, int *nfound,
                                                 const orbx_sim3_search_debug *dbg) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    OrbxSim3sPlan plan;
    const char *why = "";
    orbx_status st = orbx_sim3s_plan(nkeyframes, keyframes, nproblems, problems, camera4, bounds4, h->p.nlevels, matches12, nfound,
                                     plan, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    if (nproblems == 0) return ORBX_OK;
    OrbxSim3sCam cam;
    OrbxSim3sGrid grid;
    orbx_sim3s_camera(camera4, bounds4, h->p.fp_mode == ORBX_FP_GCC_FMA ? 1 : 0, h->p.nlevels, h->ps_thr, h->tab.scale, cam, grid);
    if (plan.nq == 0 || h->host_only || host_selected("ORBX_SIM3SEARCH")) {   // (no feature anywhere: nothing to launch)
        std::vector<uint8_t> in(plan.in_bytes), out(plan.out_bytes);
        orbx_sim3s_pack(keyframes, problems, plan, in.data());
        orbx_sim3s_host_run(plan, cam, grid, in.data(), out.data());
        orbx_sim3s_unpack(plan, in.data(), out.data(), matches12, nfound, dbg);
        return ORBX_OK;
    }
    uint8_t *pin = nullptr, *d = nullptr;
    const size_t down = dbg ? plan.out_bytes : plan.out_small;
    st = stage_begin(h, plan.in_bytes + down, plan.in_bytes + plan.dev_bytes, &pin, &d, false);
    if (st != ORBX_OK) return st;
    orbx_sim3s_pack(keyframes, problems, plan, pin);
    st = stage_upload(h, pin, d, plan.in_bytes);
    if (st != ORBX_OK) return st;
    uint8_t *dev = d + plan.in_bytes;
    { ProfScope ps(h, ORBX_K_MATCH);
      orbx_launch_sim3_search(h->stream, orbx_sim3s_args(plan, cam, d, dev), grid); }
    st = stage_download_wait(h, pin + plan.in_bytes, dev + plan.o_out, down);
    if (st != ORBX_OK) return st;
    orbx_sim3s_unpack(plan, pin, pin + plan.in_bytes, matches12, nfound, dbg);
    return ORBX_OK;
}
