// orbx_mappoint.h -- batched MapPoint::ComputeDistinctiveDescriptors / MapPoint::UpdateNormalAndDepth
// (orbx_distinctive_descriptors_batch[_device], orbx_update_normal_and_depth_batch): what the host packs and the kernels read,
// and the validation / planning / packing unit (orbx_mappoint.cpp).  No HIP in here: the unit builds alone
// (tests/san_mappoint_pack.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/orbx.h"

// Size classes of the descriptor kernels: a point with 1 .. ORBX_MP_GROUP rows is served by a group of ORBX_MP_GROUP lanes of
// k_mp_distinct (four points per wave), every larger one by a workgroup of k_mp_distinct_wide (one wave per row of D).  That
// kernel keeps a row of D in registers, ORBX_MP_SLOTS distances per lane, and the point's descriptors in LDS, while
// N <= ORBX_MP_LDS_ROWS = 64 * ORBX_MP_SLOTS; beyond that it recomputes the row from global memory in every bisection step.
enum { ORBX_MP_GROUP = 16, ORBX_MP_SLOTS = 16, ORBX_MP_LDS_ROWS = 1024 };

// Layout of one descriptor call.  Uploaded block (one copy): obs_begin[npoints + 1] | order[n_small + n_wide] (the points with
// rows, those of the small class first, each class in the caller's order) | the rows (host form: 32 bytes each; device form:
// one int64 pool row each).  Device only, after it, and downloaded in one copy of out_bytes from o_idx: best_idx[npoints] |
// best_median[npoints] | best_desc[npoints x 32].
struct OrbxMpPlan {
    int npoints = 0, n_small = 0, n_wide = 0;
    size_t nrows = 0;
    size_t o_begin = 0, o_order = 0, o_rows = 0, in_bytes = 0;
    size_t o_idx = 0, o_med = 0, o_desc = 0, out_bytes = 0, dev_bytes = 0;
};
// Validation of the whole call, before any device work, and the layout.  desc: host form; obs_row / pool_rows / d_pool: device
// form (device_form set).  ORBX_OK / ORBX_BAD_ARGUMENT / ORBX_UNSUPPORTED; *why names the offending argument.
orbx_status orbx_mp_distinct_plan(int npoints, const int32_t *obs_begin, const uint8_t *desc, bool device_form, const void *d_pool,
                                  int64_t pool_rows, const int64_t *obs_row, const int32_t *best_idx, OrbxMpPlan &plan,
                                  const char **why);
// Packing into `dst` (plan.in_bytes bytes).  The caller's arrays are not read afterwards.
void orbx_mp_distinct_pack(const int32_t *obs_begin, const uint8_t *desc, const int64_t *obs_row, const OrbxMpPlan &plan,
                           uint8_t *dst);
// The downloaded block (plan.out_bytes bytes from o_idx) into the caller's arrays: a point without rows gets best_idx =
// best_median = -1 and keeps its best_desc row.  best_median / best_desc may be NULL.
void orbx_mp_distinct_unpack(const int32_t *obs_begin, const OrbxMpPlan &plan, const uint8_t *src, int32_t *best_idx,
                             int32_t *best_median, uint8_t *best_desc);

// One point of a normal / depth call
struct DMpPoint {
    float pos[3], ref[3];     // GetWorldPos(), mpRefKF->GetCameraCenter()
    float level_scale;        // mvScaleFactors[ref_level]
    int32_t pad;
};
static_assert(sizeof(DMpPoint) == 32, "packed for the device");
// Uploaded block: obs_begin[npoints + 1] | DMpPoint[npoints] | centers[3 x nrows].  Device only, after it, downloaded in one
// copy: out[npoints][5] = normal x, y, z, min_distance, max_distance.
struct OrbxMpNormalPlan {
    int npoints = 0;
    size_t nrows = 0;
    size_t o_begin = 0, o_points = 0, o_centers = 0, in_bytes = 0, o_out = 0, out_bytes = 0, dev_bytes = 0;
};
orbx_status orbx_mp_normal_plan(int npoints, const int32_t *obs_begin, const float *pos, const float *centers,
                                const float *ref_center, const int32_t *ref_level, int nlevels, const float *normal,
                                const float *min_distance, const float *max_distance, OrbxMpNormalPlan &plan, const char **why);
void orbx_mp_normal_pack(const int32_t *obs_begin, const float *pos, const float *centers, const float *ref_center,
                         const int32_t *ref_level, const float *scale, const OrbxMpNormalPlan &plan, uint8_t *dst);
void orbx_mp_normal_unpack(const int32_t *obs_begin, const OrbxMpNormalPlan &plan, const uint8_t *src, float *normal,
                           float *min_distance, float *max_distance);
