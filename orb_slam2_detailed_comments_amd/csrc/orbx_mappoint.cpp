// orbx_mappoint.cpp -- host side of the batched MapPoint refresh (orbx_mappoint.h): validation of a call, the size-class plan
// of the descriptor kernels, the packing of the caller's arrays into one staging block and the scatter of the downloaded
// block.  HIP-free: tests/san_mappoint_pack.cpp builds it alone under the sanitizers.  The entry points (orbx_map_batches.cpp) own
// the staging block, the arena and the launches.
#include <cstring>
#include "orbx_mappoint.h"

static inline size_t mp_pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// npoints >= 1 from here on.  *nrows = obs_begin[npoints]
static orbx_status mp_ragged(int npoints, const int32_t *obs_begin, size_t *nrows, const char **why) {
    if (!obs_begin) { *why = "null obs_begin"; return ORBX_BAD_ARGUMENT; }
    if (obs_begin[0] != 0) { *why = "obs_begin[0] != 0"; return ORBX_BAD_ARGUMENT; }
    for (int p = 0; p < npoints; ++p)
        if (obs_begin[p + 1] < obs_begin[p]) { *why = "obs_begin must not decrease"; return ORBX_BAD_ARGUMENT; }
    *nrows = (size_t)obs_begin[npoints];
    return ORBX_OK;
}

orbx_status orbx_mp_distinct_plan(int npoints, const int32_t *obs_begin, const uint8_t *desc, bool device_form, const void *d_pool,
                                  int64_t pool_rows, const int64_t *obs_row, const int32_t *best_idx, OrbxMpPlan &plan,
                                  const char **why) {
    plan = OrbxMpPlan();
    if (npoints < 0) { *why = "npoints < 0"; return ORBX_BAD_ARGUMENT; }
    if (device_form && pool_rows < 0) { *why = "pool_rows < 0"; return ORBX_BAD_ARGUMENT; }
    if (npoints == 0) return ORBX_OK;
    const orbx_status st = mp_ragged(npoints, obs_begin, &plan.nrows, why);
    if (st != ORBX_OK) return st;
    if (!best_idx) { *why = "null best_idx"; return ORBX_BAD_ARGUMENT; }
    if (plan.nrows > 0) {
        if (!device_form && !desc) { *why = "null desc"; return ORBX_BAD_ARGUMENT; }
        if (device_form) {
            if (!d_pool || !obs_row) { *why = "null d_pool or obs_row"; return ORBX_BAD_ARGUMENT; }
            if ((uintptr_t)d_pool & 15) { *why = "d_pool is not 16-byte aligned"; return ORBX_BAD_ARGUMENT; }
            for (size_t t = 0; t < plan.nrows; ++t)
                if (obs_row[t] < 0 || obs_row[t] >= pool_rows) { *why = "obs_row outside [0, pool_rows)"; return ORBX_BAD_ARGUMENT; }
        }
    }
    plan.npoints = npoints;
    for (int p = 0; p < npoints; ++p) {
        const int n = obs_begin[p + 1] - obs_begin[p];
        if (n == 0) continue;
        if (n <= ORBX_MP_GROUP) ++plan.n_small; else ++plan.n_wide;
    }
    const size_t np = (size_t)npoints;
    plan.o_begin = 0;
    plan.o_order = mp_pad256((np + 1) * sizeof(int32_t));
    plan.o_rows = plan.o_order + mp_pad256(((size_t)plan.n_small + plan.n_wide) * sizeof(int32_t));
    plan.in_bytes = plan.o_rows + mp_pad256(plan.nrows * (device_form ? sizeof(int64_t) : 32));
    plan.o_idx = plan.in_bytes;
    plan.o_med = plan.o_idx + mp_pad256(np * sizeof(int32_t));
    plan.o_desc = plan.o_med + mp_pad256(np * sizeof(int32_t));
    plan.dev_bytes = plan.o_desc + mp_pad256(np * 32);
    plan.out_bytes = plan.dev_bytes - plan.o_idx;
    return ORBX_OK;
}

void orbx_mp_distinct_pack(const int32_t *obs_begin, const uint8_t *desc, const int64_t *obs_row, const OrbxMpPlan &plan,
                           uint8_t *dst) {
    if (plan.npoints <= 0) return;
    memcpy(dst + plan.o_begin, obs_begin, ((size_t)plan.npoints + 1) * sizeof(int32_t));
    int32_t *order = (int32_t *)(dst + plan.o_order);
    int ns = 0, nw = plan.n_small;
    for (int p = 0; p < plan.npoints; ++p) {
        const int n = obs_begin[p + 1] - obs_begin[p];
        if (n == 0) continue;
        if (n <= ORBX_MP_GROUP) order[ns++] = p; else order[nw++] = p;
    }
    if (plan.nrows == 0) return;
    if (obs_row) memcpy(dst + plan.o_rows, obs_row, plan.nrows * sizeof(int64_t));
    else memcpy(dst + plan.o_rows, desc, plan.nrows * 32);
}

void orbx_mp_distinct_unpack(const int32_t *obs_begin, const OrbxMpPlan &plan, const uint8_t *src, int32_t *best_idx,
                             int32_t *best_median, uint8_t *best_desc) {
    const int32_t *idx = (const int32_t *)src;
    const int32_t *med = (const int32_t *)(src + (plan.o_med - plan.o_idx));
    const uint8_t *d = src + (plan.o_desc - plan.o_idx);
    for (int p = 0; p < plan.npoints; ++p) {
        const bool live = obs_begin[p + 1] > obs_begin[p];
        best_idx[p] = live ? idx[p] : -1;
        if (best_median) best_median[p] = live ? med[p] : -1;
        if (best_desc && live) memcpy(best_desc + (size_t)p * 32, d + (size_t)p * 32, 32);
    }
}

orbx_status orbx_mp_normal_plan(int npoints, const int32_t *obs_begin, const float *pos, const float *centers,
                                const float *ref_center, const int32_t *ref_level, int nlevels, const float *normal,
                                const float *min_distance, const float *max_distance, OrbxMpNormalPlan &plan, const char **why) {
    plan = OrbxMpNormalPlan();
    if (npoints < 0) { *why = "npoints < 0"; return ORBX_BAD_ARGUMENT; }
    if (npoints == 0) return ORBX_OK;
    const orbx_status st = mp_ragged(npoints, obs_begin, &plan.nrows, why);
    if (st != ORBX_OK) return st;
    if (!pos || !ref_center || !ref_level || !normal || !min_distance || !max_distance) {
        *why = "null argument";
        return ORBX_BAD_ARGUMENT;
    }
    if (plan.nrows > 0 && !centers) { *why = "null centers"; return ORBX_BAD_ARGUMENT; }
    for (int p = 0; p < npoints; ++p)
        if (obs_begin[p + 1] > obs_begin[p] && (ref_level[p] < 0 || ref_level[p] >= nlevels)) {
            *why = "ref_level outside [0, nlevels) on a point with rows";
            return ORBX_BAD_ARGUMENT;
        }
    plan.npoints = npoints;
    const size_t np = (size_t)npoints;
    plan.o_begin = 0;
    plan.o_points = mp_pad256((np + 1) * sizeof(int32_t));
    plan.o_centers = plan.o_points + mp_pad256(np * sizeof(DMpPoint));
    plan.in_bytes = plan.o_centers + mp_pad256(plan.nrows * 3 * sizeof(float));
    plan.o_out = plan.in_bytes;
    plan.out_bytes = mp_pad256(np * 5 * sizeof(float));
    plan.dev_bytes = plan.o_out + plan.out_bytes;
    return ORBX_OK;
}

void orbx_mp_normal_pack(const int32_t *obs_begin, const float *pos, const float *centers, const float *ref_center,
                         const int32_t *ref_level, const float *scale, const OrbxMpNormalPlan &plan, uint8_t *dst) {
    if (plan.npoints <= 0) return;
    memcpy(dst + plan.o_begin, obs_begin, ((size_t)plan.npoints + 1) * sizeof(int32_t));
    DMpPoint *pt = (DMpPoint *)(dst + plan.o_points);
    for (int p = 0; p < plan.npoints; ++p) {
        DMpPoint &P = pt[p];
        for (int c = 0; c < 3; ++c) { P.pos[c] = pos[3 * (size_t)p + c]; P.ref[c] = ref_center[3 * (size_t)p + c]; }
        // the plan checked the level of every point with rows; the others are not computed
        P.level_scale = obs_begin[p + 1] > obs_begin[p] ? scale[ref_level[p]] : 0.f;
        P.pad = 0;
    }
    if (plan.nrows > 0) memcpy(dst + plan.o_centers, centers, plan.nrows * 3 * sizeof(float));
}

void orbx_mp_normal_unpack(const int32_t *obs_begin, const OrbxMpNormalPlan &plan, const uint8_t *src, float *normal,
                           float *min_distance, float *max_distance) {
    const float *out = (const float *)src;
    for (int p = 0; p < plan.npoints; ++p) {
        if (obs_begin[p + 1] == obs_begin[p]) continue;
        const float *o = out + 5 * (size_t)p;
        for (int c = 0; c < 3; ++c) normal[3 * (size_t)p + c] = o[c];
        min_distance[p] = o[3];
        max_distance[p] = o[4];
    }
}
