// orbx_handle.h -- struct orbx_handle and what every unit that touches it shares: the error record, HIPCHK, the profiling
// scope, and the staging of the host-buffer entry points (page-locked blocks, one device arena).  Internal, not installed.
// The HIP-free units (orbx_geometry.cpp, orbx_track_pack.cpp, orbx_mappoint.cpp, orbx_pose.cpp, orbx_sim3.cpp,
// orbx_pnp.cpp, orbx_init.cpp) do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "orbx_internal.h"
#include "orbx_launch.h"

orbx_status orbx_fail(orbx_status s, const std::string &msg);   // orbx_api.cpp: records orbx_last_error()
#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return orbx_fail(ORBX_HIP_ERROR, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct ProfPair { hipEvent_t a, b; int kid; };
struct orbx_handle {
    orbx_params p;
    OrbxTables tab;
    OrbxGeom geom;
    DGeom dg;
    bool host_only = false, configured = false;
    int dev = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    // side stream of the batched extraction (high priority): the small pyramid levels are a chain of short, latency-bound
    // launches; they run here, next to the issue-bound FAST kernel of the large levels on the main stream
    hipStream_t side_stream = nullptr;
    hipStream_t plan_stream = nullptr;   // side stream of the FAST-first plan (low priority: its resize chains fill what FAST leaves)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_stereo = nullptr;   // orders the batched stereo match with the OTHER eye's stream (two extractors, two streams)
    int fork_level = 0;       // first level whose resize + FAST run on the side stream (0 = no fork)
    int fork_group = 0;       // first FAST group of that level
    // sub-batch pipeline of run_chunk (ORBX_PIPELINE=0|S, ORBX_PIPELINE_HEAD=0|1, ORBX_FAST_ROOM=0|1 for A/B runs)
    int pipeline = 2;         // sub-batches of a batch of >= ORBX_PIPE_MIN_FRAMES frames (<= 1: the serial sequence)
    bool pipe_head = true;    // the first sub-batch is half the size of the others (its pyramid is the one nothing hides): the
                              // even split is 0.3 % faster on the default line but 1.8 % slower on the merged EuRoC stereo batch
    bool fast_room = false;   // k_fast_rows capped at ORBX_FAST_PIPE_WAVES waves per CU while the pipeline runs (measured slower)
    hipEvent_t ev_pipe[ORBX_PIPE_MAX] = {};   // pyramid of sub-batch k done (side stream) -> its FAST launch (main stream)
    // FAST-first plan of run_chunk (ORBX_PLAN=fastfirst|pipeline|serial, ORBX_PLAN_SUB=S, ORBX_PLAN_HEAD=0|1, ORBX_PLAN_MIN_FRAMES;
    // ORBX_PLAN_PRIORITY=low|normal|high is read when the handle is created);
    // an explicit ORBX_PIPELINE overrides ORBX_PLAN and selects the serial sequence or the sub-batch pipeline as they were
    bool fast_first = true;   // the default plan of a batch of >= plan_min_frames frames (profiles/fast_first_plan.md)
    int plan_sub = 3;         // resize-chain sub-batches of the plan (the sweep of profiles/fast_first_plan.md)
    bool plan_head = false;   // the first of them is half the size of the others
    int plan_min_frames = ORBX_PIPE_MIN_FRAMES;   // smaller batches keep the serial sequence
    int l0_groups = 0;        // FAST groups of level 0 (the groups are ordered by level)
    int max_ch_l0 = 0, max_ch_rest = 0;   // tallest cell of the level-0 groups / of the others
    // geometry-dependent device state
    uint8_t *d_pyr = nullptr, *d_blur = nullptr;
    OrbxCell *d_cells = nullptr;
    OrbxFastGroup *d_groups = nullptr;
    bool resize_legacy = false;   // ORBX_RESIZE_IMPL=legacy: k_pyr_resize for every level (A/B runs)
    int rr_rpw = 0;               // ORBX_RR_RPW: destination rows per wave of the row-walking resize kernels (2..64, a power of two); 0 = the launcher's choice
    int match_kernel = 0;        // ORBX_MATCH_KERNEL, read ONCE when the handle is created: 0 = matrix pipe with FP4 operands (default), 1 = "valu" (vector pipe), 2 = "i8" (matrix pipe, int8 operands) -- A/B runs, parity tests
    int fast_stop = 0;      // ORBX_FAST_STOP: only read in -DORBX_TIMING_KNOBS builds
    int fast_lcap = 640;    // LDS work-list entries of k_fast_rows (ORBX_FAST_LCAP; tests shrink it to force the flush paths)
    int fast_gpw = 0;       // ORBX_FAST_GPW: groups per wave of k_fast_rows forced to 1 or 2 (tests pair planted groups at small batches); 0 = the launcher's size rule
    OrbxTap *d_taps = nullptr;
    uint2 *d_dense = nullptr;   // dense per-(frame, level) key arrays, appended to by k_fast_rows (fill counts in d_cand_count)
    int *d_cand_count = nullptr, *d_lvl_count = nullptr, *d_status = nullptr;
    uint32_t *d_lvl_kp = nullptr;
    float *d_lvl_angle = nullptr;
    uint16_t *d_knode = nullptr;
    int max_cw = 0, max_ch = 0, ncap = 0, lds_keys = 0, lds_keys_few = 0, qt_reg_keys = 0;
    // staging for the host entry points
    uint8_t *st_in[2] = {nullptr, nullptr}; size_t d_in_bytes = 0;
    orbx_keypoint *st_kps[2] = {nullptr, nullptr}; uint8_t *st_desc[2] = {nullptr, nullptr}; int *st_cnt[2] = {nullptr, nullptr};
    int out_cap = 0, stage_chunk = 0;
    int *pin_stat = nullptr; size_t pin_stat_ints = 0;   // page-locked landing place of the per-frame counts | status words of a call (grow-only)
    hipStream_t s_in = nullptr;   // the ONE copy stream of the pipelined host-buffer call (uploads and downloads in turn)
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    // staging of orbx_extract_rgbd_batch (grow-only): the depth frames of a chunk; kps_un | u_right | depth of a chunk (one block)
    uint8_t *st_dep[2] = {nullptr, nullptr}; size_t dep_bytes = 0;
    uint8_t *st_rg[2] = {nullptr, nullptr}; size_t rg_bytes = 0;
    int last_batch = 0;
    int mk_w = 0, mk_h = 0, mk_total = 0;   // orbx_max_keypoints cache
    void *d_match_ws = nullptr; size_t match_ws_bytes = 0;   // partial (best, second) keys of k_match
    uint32_t *d_gate_items = nullptr; size_t gate_items_cap = 0;   // candidate lists of k_gate / distance blocks of k_block_dist (grow-only)
    size_t gate_guess = 4096;                                      // entries the speculative download of the candidate lists covers
    // page-locked staging of the host-buffer entry points (not the pipelined extraction): two grow-only blocks, one growth rule.
    // `pin`: the calls that wait for the stream before they return, so it is free whenever a call begins.  `pin_early`: the calls
    // that return before their upload has run (batched tracking): not written again before the event behind that upload has passed.
    uint8_t *pin = nullptr; size_t pin_bytes = 0;
    uint8_t *pin_early = nullptr; size_t pin_early_bytes = 0;
    hipEvent_t ev_stage = nullptr; bool stage_pending = false, stage_early = false;   // stage_early: the block of the call in progress
    // MapPoint::PredictScale as thresholds on mfMaxDistance / dist (orbx_track.h: orbx_predict_scale_build), built at orbx_create
    float ps_thr[ORBX_PS_LEVELS] = {};
    // grow-only scratch arena for the host-buffer convenience entry points (match / matrix / stereo): no hipMalloc
    // on the steady-state path and nothing to leak on an error return
    uint8_t *d_scratch = nullptr; size_t scratch_bytes = 0, scratch_used = 0;
    uint2 *d_rect = nullptr; int rect_w = 0, rect_h = 0;   // pre-digested rectification maps (orbx_set_rectification)
    int input_format = ORBX_FMT_GRAY8;        // pixel format of the frames handed to the extract entry points
    bool blur_valid = false;                // d_blur holds the blurred pyramid of the last batch
    // in-place level 0 (orbx_inplace.h): grey batches of orbx_extract_batch_device read level 0 from the caller's image and
    // never write the slab's padded copy; whoever needs that copy afterwards calls ensure_level0() first
    bool l0_inplace = true;                 // ORBX_LEVEL0_INPLACE=0 forces the eager k_pyr_l0 everywhere (A/B runs)
    bool l0_eager_sticky = false;           // a stereo match needed the padded copy: this handle's later batches write it eagerly
    bool l0_pending = false;                // the slab's level 0 of the last batch has not been written
    OrbxRaw0 l0_src = {nullptr, 0, 0, 0, 0};   // ... and this is the input it would be written from (must stay valid and unchanged)
    int *d_l0_scratch = nullptr;            // status / cursor words the late k_pyr_l0 may reset instead of the batch's own
    // profiling
    uint32_t prof_mask = 0;
    std::vector<ProfPair> pending;
    std::vector<hipEvent_t> pool;
    float ms[ORBX_K_COUNT] = {0};
    int launches[ORBX_K_COUNT] = {0};
};

// roctx ranges around every stage's launches (orbx_api.cpp: Roctx); push returns false when they are switched off
bool orbx_roctx_push(const char *name) __attribute__((visibility("hidden")));
void orbx_roctx_pop() __attribute__((visibility("hidden")));
struct ProfScope {
    orbx_handle *h; int kid; bool on; hipStream_t st; hipEvent_t a = nullptr, b = nullptr; bool marked = false;
    ProfScope(orbx_handle *h_, int kid_, hipStream_t st_ = nullptr)
        : h(h_), kid(kid_), on(((h_->prof_mask >> kid_) & 1u) != 0), st(st_ ? st_ : h_->stream) {
        marked = orbx_roctx_push(orbx_kernel_name(kid));
        if (!on) return;
        a = grab(); b = grab();
        hipEventRecord(a, st);   // events are recorded on the stream the kernel is launched on
    }
    hipEvent_t grab() {
        if (!h->pool.empty()) { hipEvent_t e = h->pool.back(); h->pool.pop_back(); return e; }
        hipEvent_t e; hipEventCreate(&e); return e;
    }
    ~ProfScope() {
        if (marked) orbx_roctx_pop();
        if (!on) return;
        hipEventRecord(b, st);
        h->pending.push_back({a, b, kid});
    }
};

#pragma GCC visibility push(hidden)   // what follows is shared between the library's own units only: not exported
void prof_drain(orbx_handle *h);
orbx_status configure(orbx_handle *h, int width, int height);   // orbx_api.cpp: the handle's geometry and device buffers for one image size
// ORBX_FAST_GPW into h->fast_gpw (0 when unset; anything but 1 or 2 is ORBX_BAD_ARGUMENT): configure(), and orbx_debug_fast_gpw on
// a handle that has not been configured (a host-only one never is)
orbx_status read_fast_gpw(orbx_handle *h);
// ---------------------------------------------------------------- staging (orbx_api.cpp)
// A grow-only device buffer: *cap < need frees it behind a wait for the handle's stream and allocates `want` elements (contents go).
orbx_status dev_grow(orbx_handle *h, void **p, size_t *cap, size_t need, size_t want, size_t elem = 1);
// The device arena: reserve restarts it (and grows it), take hands out 256-byte aligned pieces of what was reserved.
orbx_status scratch_reserve(orbx_handle *h, size_t bytes);
template <typename T> static T *scratch_take(orbx_handle *h, size_t count) {
    T *p = (T *)(h->d_scratch + h->scratch_used);
    h->scratch_used += (count * sizeof(T) + 255) & ~(size_t)255;
    return p;
}
static inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }
// h->pin at least `bytes` large (contents go when it grows): for the two calls that size it apart from their arena.
orbx_status stage_pin(orbx_handle *h, size_t bytes);
// A staged call begins: sets the device; *pin = h->pin, or for a call that returns without a wait for the stream (returns_early)
// h->pin_early behind a wait for a pending upload; *dev = a fresh arena.  The handle remembers which block the call took.
orbx_status stage_begin(orbx_handle *h, size_t pin_bytes, size_t dev_bytes, uint8_t **pin, uint8_t **dev, bool returns_early);
// The upload of the call stage_begin began; where that call returns early, records the copy's event and marks its block pending.
orbx_status stage_upload(orbx_handle *h, const uint8_t *pin, uint8_t *dev, size_t bytes);
// One download into the block behind the launches so far, and the wait for it (any launch error surfaces here).
orbx_status stage_download_wait(orbx_handle *h, uint8_t *pin, const uint8_t *d_out, size_t bytes);
static inline bool grid_params(float min_x, float max_x, float min_y, float max_y, DGrid &gp) {
    if (!(max_x > min_x) || !(max_y > min_y)) return false;
    gp.minx = min_x; gp.miny = min_y;
    gp.winv = 64.0f / (max_x - min_x);     // mfGridElementWidthInv (src/Frame.cc:96-99): FRAME_GRID_COLS / (mnMaxX - mnMinX)
    gp.hinv = 48.0f / (max_y - min_y);
    return true;
}
#pragma GCC visibility pop
