// orbx_track.h -- batched, device-resident SearchByProjection of the two tracking matchers
// (orbx_search_by_projection_frame_batch_device / orbx_search_by_projection_mappoints_batch_device): the records the host packs
// and the kernels read, and the packing / validation unit (orbx_track_pack.cpp).  No HIP in here: the packing unit builds alone
// (tests/san_track_pack.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/orbx.h"

// One point of one problem.  Map-point policy: the GetFeaturesInArea query as it is (x, y = mTrackProjX / Y, ur = mTrackProjXR,
// r = the window, level band).  Frame policy: as packed, (x, y, ur) is the MapPoint's world position and min_level the
// last-frame octave; k_track_project turns the record into the query in place (projection, u_right prediction, octave band) or
// switches it off.  r < 0: the point takes no part.
struct DTrackQ {
    float x, y, ur, r;
    int32_t min_level, max_level;
    int32_t obs;      // Observations() of the point's MapPoint: > 0 blocks the feature it is assigned to
    float angle;      // LastFrame.mvKeysUn[i].angle (frame policy)
    int32_t prob, pad;
};
// One problem: its frame of the device batch, its points q[q_begin .. q_begin + nq), and (frame policy) the pose of the
// current frame with the direction of motion: dir = 1 forward, 2 backward, 0 neither (src/ORBmatcher.cc:1731-1732)
struct DTrackProb {
    int32_t frame, q_begin, nq, dir;
    float Rcw[9], tcw[3];
};
static_assert(sizeof(DTrackQ) == 40 && sizeof(DTrackProb) == 64, "packed for the device");

// Layout of one call.  Uploaded block (one copy): problems | points | point descriptors | blocked-feature seeds (map-point
// policy: one bitmap of `seed_words` words per problem, bit i = frame_observations[i] > 0).  Device only, after it: the stored
// candidates (one uint4 per point) | the accept events (one int per point).
struct OrbxTrackPlan {
    int nproblems = 0, seed_words = 0;
    size_t nq = 0;
    size_t o_prob = 0, o_q = 0, o_desc = 0, o_seed = 0, in_bytes = 0, o_cand = 0, o_ev = 0, dev_bytes = 0;
};
struct OrbxTrackBatchArgs { int nframes, cap, nlevels; bool device_pointers_ok; };

// Validation of the whole call, before any device work, and the layout.  ORBX_OK / ORBX_BAD_ARGUMENT / ORBX_UNSUPPORTED; *why
// names the offending argument.
orbx_status orbx_track_frame_plan(int nproblems, const orbx_track_frame_problem *problems, const OrbxTrackBatchArgs &a,
                                  OrbxTrackPlan &plan, const char **why);
orbx_status orbx_track_points_plan(int nproblems, const orbx_track_points_problem *problems, const OrbxTrackBatchArgs &a,
                                   OrbxTrackPlan &plan, const char **why);
// Packing into `dst` (plan.in_bytes bytes); scale = mvScaleFactors of the handle.  The caller's arrays are not read afterwards.
void orbx_track_frame_pack(int nproblems, const orbx_track_frame_problem *problems, const OrbxTrackPlan &plan, const float *scale,
                           float mb, uint8_t *dst);
void orbx_track_points_pack(int nproblems, const orbx_track_points_problem *problems, const OrbxTrackPlan &plan, const float *scale,
                            int cap, uint8_t *dst);
