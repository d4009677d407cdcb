// orbx_launch.h -- kernel launch wrappers (defined in orbx_kernels.hip, used by the C ABI units)
#pragma once
#include <hip/hip_runtime.h>
#include "orbx_device.h"
#include "orbx_inplace.h"
#include "orbx_track.h"
#include "orbx_mappoint.h"
#include "orbx_pose.h"
#include "orbx_sim3opt.h"
#include "orbx_localba.h"
#include "orbx_essgraph.h"
#include "orbx_sim3.h"
#include "orbx_pnp.h"
#include "orbx_init.h"
#include "orbx_recon.h"
#include "orbx_newpoints.h"
#include "orbx_sim3search.h"

// ---- launch regimes chosen from the size of a launch alone: ONE definition, used by the launchers (orbx_kernels.hip) and
// reported by orbx_debug_match_plan / orbx_debug_fast_gpw, so that a test can assert the regime it is running in
#define MT_SPLIT 16     // most ways the train set is split over blockIdx.y; partials merged by k_match_merge.  The launcher picks
                        // the smallest split that still fills the chip (every extra split repeats the query expansion and
                        // one partial record per query)
#define MT_QPW(QT) (32 * (QT))   // queries per wave of k_match / k_match_f4: QT column tiles of 32
#ifndef FR_GPW
#define FR_GPW 2        // groups per wave of k_fast_rows in a launch with waves to spare
#endif
// orbx_launch_match.  kernel: 0 = matrix pipe, FP4 operands (default); 1 = vector pipe (ORBX_MATCH_KERNEL=valu); 2 = matrix pipe,
// int8 operands (=i8).  qt = query tiles per wave of the matrix-pipe kernels (0: the vector-pipe kernel); nsplit = blocks the
// train set of a pair is split over (nsplit == 1 on the matrix pipe: direct output, no k_match_merge)
struct OrbxMatchPlan { int qt, nsplit; };
static inline OrbxMatchPlan orbx_match_plan(int npairs, int max_nq, int kernel) {
    auto split = [](long long waves, long long base) {
        const long long n = waves / base;
        return (int)(n < 1 ? 1 : n > MT_SPLIT ? MT_SPLIT : n);
    };
    if (kernel == 1) {   // 128 queries per wave; the split that reaches ~16384 waves
        const long long base = (long long)((max_nq + 127) / 128) * npairs;
        return {0, split(16384 + base - 1, base)};
    }
    // 512 queries per block (QT = 4, two waves per SIMD: the chip holds 2048 such waves) when the launch fills the chip that
    // way without splitting the train set; otherwise 256 per block and the train split that reaches ~4096 waves
    const long long waves4 = (long long)((max_nq + MT_QPW(4) - 1) / MT_QPW(4)) * npairs;
    if (waves4 >= 2048) return {4, 1};
    return {2, split(4096, (long long)((max_nq + MT_QPW(2) - 1) / MT_QPW(2)) * npairs)};
}
// orbx_launch_fast_rows, groups per wave: FR_GPW when the launch has waves to spare (the second group's tile is prefetched while
// the first is processed); one per wave for small batches, where the serial length of a wave is what the caller waits for.
// forced = 1 or 2 (ORBX_FAST_GPW, tests) overrides the size rule; 0 = the size rule.
static inline int orbx_fast_gpw(int B, int ngroups, int forced) {
    return forced > 0 ? forced : (long long)B * ngroups >= 16384 ? FR_GPW : 1;
}

hipError_t orbx_upload_pattern();
// the per-lane pattern tables, 64 lanes x 16 coordinates each (host only): orbx_upload_pattern uploads the int8 one (c_pattern_lane);
// the same coordinates as floats serve the debug entry orbx_debug_describe_pattern
void orbx_pattern_lane_tables(signed char *i8, float *f32);
size_t orbx_quadtree_smem(int ncap, int lds_keys);
hipError_t orbx_quadtree_prepare(size_t smem);
void orbx_launch_clear(hipStream_t s, int *a, int na, int *b, int nb, int *c, int nc);
void orbx_launch_pyr_l0(hipStream_t s, const DGeom &g, int B, const uint8_t *imgs, int W, int H, int stride,
                        long long frame_stride, uint8_t *pyr, int *status, int *cand_cursor);
void orbx_launch_pyr_l0_color(hipStream_t s, const DGeom &g, int B, const uint8_t *imgs, int W, int H, int stride,
                              long long frame_stride, uint8_t *pyr, int nch, int r_off, int b_off, int *status, int *cand_cursor);
void orbx_launch_pyr_l0_remap(hipStream_t s, const DGeom &g, int B, const uint8_t *imgs, int W, int H, int stride,
                              long long frame_stride, uint8_t *pyr, const uint2 *rect, int *status, int *cand_cursor);
void orbx_launch_pyr_resize(hipStream_t s, const DGeom &g, int B, int level, const OrbxTap *taps, uint8_t *pyr, bool narrow,
                            int rpw_forced = 0);
// (rpw_forced > 0: destination rows per wave of the row-walking kernel, a power of two in 2..64 -- ORBX_RR_RPW; 0: the launcher's choice)
void orbx_launch_fast_rows(hipStream_t s, const DGeom &g, int B, const OrbxCell *cells, const OrbxFastGroup *groups,
                           int ngroups, const uint8_t *pyr, uint2 *cand, int *cand_cursor, int *status, int max_ch, int lcap,
                           int dbg_stop, int lds_floor = 0, const OrbxRaw0 *raw = nullptr, bool l0_only = false,
                           int gpw_forced = 0);
// (raw: the level-0 groups read the caller's image; l0_only with raw: every group of the launch is a level-0 group.  max_ch is
// the tallest cell of the groups of THIS launch: it sizes the LDS tile and score map.  gpw_forced: orbx_fast_gpw above.)
// in-place mode (orbx_inplace.h): level 1 from the caller's grey image `raw`; also resets status[f] and cand_cursor[f][*] as
// k_pyr_l0 does, unless `status` is null (the FAST-first plan resets them before its first FAST launch).  taps_l1 = the level's raw-coordinate tap table (pw horizontal records, then ph vertical ones).
void orbx_launch_pyr_resize_l1(hipStream_t s, const DGeom &g, int B, const OrbxTap *taps_l1, const OrbxRaw0 &raw, uint8_t *pyr,
                               int tail_bx, int *status, int *cand_cursor, int rpw_forced = 0);
void orbx_launch_undistort(hipStream_t s, int B, int max_n, int cap, const double *K4, const double *k14, int identity,
                           const orbx_keypoint *kps, const int *counts, orbx_keypoint *out);
// depth input of k_rgbd (Frame::ComputeStereoFromRGBD): `depth` = frame 0, frames `frame_stride` bytes apart, rows `stride`
// bytes apart; scale_f32 = f32 input that Tracking::GrabImageRGBD converts in place (|scale - 1| > 1e-5)
struct OrbxRgbdArgs {
    const uint8_t *depth; long long frame_stride, stride;
    int format, width, height, scale_f32;
    float scale, mbf;
};
void orbx_launch_rgbd(hipStream_t s, int B, int max_n, int cap, const double *K4, const double *k14, int identity,
                      const OrbxRgbdArgs &a, const orbx_keypoint *kps, const orbx_keypoint *kun_in, const int *counts,
                      orbx_keypoint *kun_out, float *u_right, float *depth);
void orbx_launch_bow_transform(hipStream_t s, int B, int max_n, const int *child_begin, const uint32_t *child_ids,
                               const uint8_t *node_desc, int n_nodes, int L, const uint8_t *desc, const int *counts,
                               long long frame_stride, int levelsup, uint32_t *out_leaf, uint32_t *out_nid, int out_stride);
void orbx_launch_quadtree(hipStream_t s, const DGeom &g, int B, const uint2 *dense, const int *cand_count, uint32_t *lvl_kp, int *lvl_count,
                          int *status, uint16_t *knode_glob, int ncap, int lds_keys, int reg_keys, int level_begin, int level_count);
void orbx_launch_blur(hipStream_t s, const DGeom &g, int B, const uint8_t *pyr, uint8_t *blur);
void orbx_launch_describe(hipStream_t s, const DGeom &g, int B, const uint8_t *pyr, const uint32_t *lvl_kp,
                          const int *lvl_count, float *lvl_angle, orbx_keypoint *kps, uint8_t *desc,
                          int *counts, int *status, int cap, const OrbxRaw0 *raw = nullptr);
void orbx_launch_match(hipStream_t s, int npairs, int max_nq, const uint8_t *q, const int *nq, long long q_stride,
                       const uint8_t *t, const int *nt, long long t_stride, int *best_idx, int *best_dist,
                       int *second_dist, int out_stride, void *workspace, int kernel);
size_t orbx_match_workspace_bytes(int npairs, int out_stride);
void orbx_launch_grid_build(hipStream_t s, const DGrid &gp, int nframes, const orbx_keypoint *kps, const int *counts, int fixed_n,
                            int cap, int *cell_begin, uint16_t *items);
void orbx_launch_gate(hipStream_t s, const DGrid &gp, const orbx_keypoint *kps, const uint8_t *desc, const int *cell_begin,
                      const uint16_t *items, const DGateQuery *q, const uint8_t *qdesc, int nq, uint2 *span, uint32_t *cursor,
                      uint32_t *out_items, uint32_t cap, int fstride);
void orbx_launch_block_dist(hipStream_t s, const uint8_t *d1, const uint8_t *d2, const DDistRow *rows, const uint32_t *col_idx,
                            int nrows, uint16_t *out);
// batched SearchByBoW: selection, one wave per DBowItem (`words` = LDS bitmap words per wave, >= ceil(max ncol / 32)), then
// the rotation check and the counts, one workgroup per problem (outputs nout entries apart)
void orbx_launch_bow_select(hipStream_t s, bool kk, const DBowItem *items, int nitems, const uint32_t *idx, const uint8_t *desc,
                            const uint8_t *hmp, float nnratio, int words, int32_t *out);
void orbx_launch_bow_rot(hipStream_t s, bool kk, int nproblems, int nout, const uint32_t *cand_base, const float *ang, int check,
                         int32_t *out, int32_t *counts);
// batched tracking matchers (orbx_track.h).  OrbxTrackFrames = the device batch the problems' current frames live in: keypoints,
// descriptors, u_right (nullptr: all -1) and counts of `cap`-strided frames, their grids, the image bounds.
struct OrbxTrackFrames {
    DGrid gp; float bounds[4];
    const orbx_keypoint *kps; const uint8_t *desc; const float *ur; const int *counts; int cap;
    const int *cell_begin; const uint16_t *items;
};
// frame policy: the packed points (world positions) become queries in place
void orbx_launch_track_project(hipStream_t s, const OrbxTrackFrames &F, const float *camera4, float mbf, int fma_mode,
                               const DTrackProb *probs, DTrackQ *q, int nq);
// k_track_frustum: isInFrustum + PredictScale + the window of the map-point policy for every (problem, point) of a local-points
// call; thr / scale = the handle's PredictScale thresholds (ORBX_PS_LEVELS entries) and mvScaleFactors
void orbx_launch_track_frustum(hipStream_t s, const OrbxTrackFrames &F, const float *camera4, float mbf, int fma_mode, int nlevels,
                               const float *thr, const float *scale, int nproblems, int max_points, const DTrackProb *probs,
                               const DTrackLocal *locals, const DTrackPoolPt *pool, const uint8_t *pdesc, const int32_t *index,
                               const uint8_t *skip, DTrackQ *q, uint8_t *qdesc, uint8_t *in_view, orbx_track_state *track);
// one wave per point: the smallest key (two = the two smallest, map-point policy) of its window -> cand[point]
void orbx_launch_track_cand(hipStream_t s, bool two, const OrbxTrackFrames &F, const DTrackProb *probs, const DTrackQ *q,
                            const uint8_t *qdesc, int nq, uint4 *cand);
// one wave per problem: the ordered selection (mp = map-point policy: seeds, ratio test; otherwise TH_HIGH and the rotation
// check over the accept events `ev`), outputs out[nproblems][cap] / nmatches[nproblems]
void orbx_launch_track_select(hipStream_t s, bool mp, const OrbxTrackFrames &F, int nproblems, const DTrackProb *probs, const DTrackQ *q,
                              const uint8_t *qdesc, const uint4 *cand, const uint32_t *seed, float nnratio, int check, int32_t *ev,
                              int32_t *out, int32_t *nmatches);
// batched MapPoint refresh (orbx_mappoint.h).  order = the points with rows, n_small of the lane-group class (k_mp_distinct) and
// behind them n_wide of the workgroup class (k_mp_distinct_wide); obs_row == nullptr: row t is desc + 32 t, otherwise desc is the
// pool and row t is desc + 32 obs_row[t].  out = 5 floats per point (normal, min_distance, max_distance).
void orbx_launch_mp_distinct(hipStream_t s, const int32_t *obs_begin, const uint8_t *desc, const int64_t *obs_row,
                             const int32_t *order, int n_small, int n_wide, int32_t *best_idx, int32_t *best_median,
                             uint8_t *best_desc);
void orbx_launch_mp_normal_depth(hipStream_t s, const int32_t *obs_begin, const DMpPoint *pts, const float *centers, int npoints,
                                 float scale_last, float *out);
void orbx_launch_pose_opt(hipStream_t s, const DPoseArgs &a);
// Optimizer::OptimizeSim3 (orbx_sim3opt.h): k_sim3_opt, one wave per problem
void orbx_launch_sim3_opt(hipStream_t s, const DSim3OptArgs &a);
// Optimizer::LocalBundleAdjustment (orbx_localba.h): k_local_ba, one workgroup per problem
void orbx_launch_local_ba(hipStream_t s, const DLbaArgs &a);
// Optimizer::OptimizeEssentialGraph (orbx_essgraph.h): k_essential_graph, one workgroup per problem, then k_eg_correct_points
void orbx_launch_essential_graph(hipStream_t s, const DEgArgs &a);
// Sim3Solver RANSAC (orbx_sim3.h): k_sim3_hypotheses over all iterations, then k_sim3_inliers over the workgroup table
void orbx_launch_sim3(hipStream_t s, const DSim3Args &a);
// PnPsolver RANSAC (orbx_pnp.h): k_pnp_hypotheses over all iterations, then k_pnp_inliers over the workgroup table
void orbx_launch_pnp(hipStream_t s, const DPnpArgs &a);
// Initializer H / F RANSAC (orbx_init.h): k_init_hypotheses over all hypotheses, then k_init_scores over the workgroup table
void orbx_launch_init(hipStream_t s, const DInitArgs &a);
// ReconstructH / ReconstructF (orbx_recon.h): k_init_decompose over the problems, k_init_check_rt over the pose hypotheses, k_init_pick
void orbx_launch_recon(hipStream_t s, const DReconArgs &a);
// the fused call, between orbx_launch_init and orbx_launch_recon: k_init_select, one wave per problem of the RANSAC
void orbx_launch_init_select(hipStream_t s, const DInitArgs &i, const DReconArgs &a);
// CreateNewMapPoints, the per-match geometry (orbx_newpoints.h): k_new_points over the chunk table, one wave per chunk
void orbx_launch_new_points(hipStream_t s, const DNewPtsArgs &a);
// SearchBySim3 batched (orbx_sim3search.h): k_grid_build over the pool, k_sim3s_project, k_sim3s_cand over the live queries, k_sim3s_mutual
void orbx_launch_sim3_search(hipStream_t s, const DSim3sArgs &a, const OrbxSim3sGrid &g);
void orbx_launch_hamming_matrix(hipStream_t s, const uint8_t *q, int nq, const uint8_t *t, int nt, uint16_t *dist);

void orbx_launch_stereo_batch(hipStream_t s, const OrbxStereoGeom &sg, int npairs, int cap, const orbx_keypoint *kL,
                              const uint8_t *dL, const int *nL, const orbx_keypoint *kR, const uint8_t *dR, const int *nR,
                              const uint8_t *pyrL, const uint8_t *pyrR, long long pyr_bytes, float *uRight, float *depth,
                              int *sad, int *nmatches, int *row_begin, uint2 *row_items);
int orbx_stereo_items_per_pair(const OrbxStereoGeom &sg, int cap);
void orbx_launch_stereo(hipStream_t s, const OrbxStereoGeom &sg, const orbx_keypoint *kL, const uint8_t *dL, int nL,
                        const orbx_keypoint *kR, const uint8_t *dR, int nR, const uint8_t *pyrL, const uint8_t *pyrR,
                        float *uRight, float *depth, int *sad, int *row_begin, uint2 *row_items);
// keyframe database (orbx_kfdb.cpp): common words of queries [q0, q0 + nq) with every slot (records appended at *cursor, the
// maximum over unconnected sharers in qmax[q]), then the scores of the records above the word threshold
void orbx_launch_kfdb_common(hipStream_t s, const uint2 *slots, int nslots, const uint32_t *pool_w, const uint32_t *qw_all,
                             const int *q_begin, int q0, int nq, const uint8_t *connected, int *qmax, uint32_t *cursor,
                             DKfRec *rec, uint32_t cap);
void orbx_launch_kfdb_score(hipStream_t s, DKfRec *rec, const uint32_t *cursor, uint32_t cap, const int *qmax, const uint2 *slots,
                            const uint32_t *pool_w, const double *pool_v, const uint32_t *qw_all, const double *qv_all,
                            const int *q_begin, int scoring, int fma_mode);
void orbx_launch_kfdb_score_slots(hipStream_t s, const uint32_t *slot_list, int n, const uint2 *slots, const uint32_t *pool_w,
                                  const double *pool_v, const uint32_t *qw, const double *qv, int nq, int scoring, int fma_mode,
                                  double *out);
