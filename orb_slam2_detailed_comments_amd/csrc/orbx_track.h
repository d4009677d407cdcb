// orbx_track.h -- batched, device-resident SearchByProjection of the two tracking matchers
// (orbx_search_by_projection_frame_batch_device / orbx_search_by_projection_mappoints_batch_device) and of
// Tracking::SearchLocalPoints whole (orbx_search_local_points_batch_device): the records the host packs
// and the kernels read, and the packing / validation unit (orbx_track_pack.cpp).  No HIP in here: the packing unit builds alone
// (tests/san_track_pack.cpp, tests/san_local_pack.cpp).
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

// ---- orbx_search_local_points_batch_device: Frame::isInFrustum + MapPoint::PredictScale in front of the map-point policy.
// One point of the local-map pool, shared by all problems of a call; its descriptor is row `index` of the pool's descriptors.
struct DTrackPoolPt {
    float P[3], Pn[3];     // GetWorldPos(), GetNormal()
    float dmin, dmax;      // mfMinDistance, mfMaxDistance (raw)
    int32_t obs;           // Observations()
};
// What k_track_frustum reads of a problem beside its DTrackProb (frame, q_begin, nq, Rcw, tcw)
struct DTrackLocal {
    float Ow[3], th, cos_limit;
    int32_t pad[3];
};
static_assert(sizeof(DTrackPoolPt) == 36 && sizeof(DTrackLocal) == 32, "packed for the device");
// Layout of one call.  Uploaded block (one copy): problems | their DTrackLocal | pool points | pool descriptors | per query the
// pool index | per query the skip flag | blocked-feature seeds.  Device only, after it: the queries k_track_frustum writes
// (DTrackQ) | their gathered descriptors | stored candidates | accept events.
struct OrbxLocalPlan {
    int nproblems = 0, seed_words = 0, npool = 0, max_points = 0;
    size_t nq = 0;
    size_t o_prob = 0, o_local = 0, o_pool = 0, o_pdesc = 0, o_index = 0, o_skip = 0, o_seed = 0, in_bytes = 0;
    size_t o_q = 0, o_desc = 0, o_cand = 0, o_ev = 0, dev_bytes = 0;
};
orbx_status orbx_track_local_plan(int nproblems, const orbx_track_local_problem *problems, const orbx_local_map_view *map,
                                  const OrbxTrackBatchArgs &a, OrbxLocalPlan &plan, const char **why);
void orbx_track_local_pack(int nproblems, const orbx_track_local_problem *problems, const orbx_local_map_view *map,
                           const OrbxLocalPlan &plan, int cap, uint8_t *dst);

// ---- MapPoint::PredictScale as a table (include/orbx.h: orbx_predict_scale_table).  thr[0] = 0, thr[k] = the smallest positive
// finite float ratio whose level (int)ceilf(logf(ratio) / logf(scale_factor)) is >= k, +inf where none is; `thr` holds
// ORBX_PS_LEVELS entries, those from nlevels on are +inf.
enum { ORBX_PS_LEVELS = 16 };
void orbx_predict_scale_build(float scale_factor, int nlevels, float *thr);
// the number of k in [1, nlevels) with ratio >= thr[k]
static inline int orbx_predict_scale_level(const float *thr, int nlevels, float ratio) {
    int lvl = 0;
    for (int k = 1; k < nlevels; ++k) lvl += ratio >= thr[k] ? 1 : 0;
    return lvl;
}
