// orbx_extract.cpp -- everything Frame::Frame does, behind the C ABI: rectification and input format, the launch plan of one
// batched extraction (run_chunk), the device and host-buffer batch calls with their pipelined staging, the RGB-D calls
// (Frame::ComputeStereoFromRGBD), and Frame::UndistortKeyPoints / ComputeImageBounds.
//
// run_chunk per batch (no host synchronisation in the device entry point): level 0 (or none, in place) -> resize chain ->
// FAST -> quadtree -> descriptors + assembly; large batches overlap the resize chains with FAST on a second stream.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>
#include "orbx_handle.h"
#include "../../include/orbx_rect_digest.h"

// orbx_extract_rgbd_batch with page-locked, device-mapped depth: read it in place (true) or upload it (false) by default;
// ORBX_RGBD_DEPTH=upload|inplace overrides per call.  Measured at 640x480, chunks of 64: 46.8 k / 49.2 k frames/s per 256 /
// 1024-frame call in place against 33.4 k / 34.7 k uploaded (profiles/rgbd_rates.log)
#define ORBX_RGBD_INPLACE_DEFAULT true

// ---------------------------------------------------------------- extraction
static inline int orbx_fmt_channels(int fmt) { return fmt == ORBX_FMT_GRAY8 ? 1 : (fmt == ORBX_FMT_RGB8 || fmt == ORBX_FMT_BGR8) ? 3 : 4; }
// cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) of Examples/Stereo/stereo_euroc.cc:183-194 in front of the extractor:
// the float maps are digested once (include/orbx_rect_digest.h: the 32-bit cvRound(map * 32), split into integer part and
// 5-bit fractions, as remap() does per block) and level 0 samples the raw image through them.  NULL maps switch the
// rectification off.
extern "C" orbx_status orbx_set_rectification(orbx_handle *h, const float *map_x, const float *map_y, int width, int height) {
    if (!h || h->host_only) return orbx_fail(h ? ORBX_NO_DEVICE : ORBX_BAD_ARGUMENT, "no device handle");
    HIPCHK(hipSetDevice(h->dev));
    HIPCHK(hipStreamSynchronize(h->stream));
    hipFree(h->d_rect); h->d_rect = nullptr; h->rect_w = h->rect_h = 0;
    if (!map_x && !map_y) return ORBX_OK;
    if (!map_x || !map_y || width <= 0 || height <= 0) return orbx_fail(ORBX_BAD_ARGUMENT, "bad rectification maps");
    if (h->input_format != ORBX_FMT_GRAY8) return orbx_fail(ORBX_BAD_ARGUMENT, "rectification needs 8-bit gray input");
    std::vector<uint2> t((size_t)width * height);
    static_assert(sizeof(uint2) == 2 * sizeof(uint32_t), "interleaved digest");
    orbx_rect_digest(map_x, map_y, t.size(), &t[0].x, &t[0].y, 2);
    HIPCHK(hipMalloc(&h->d_rect, t.size() * sizeof(uint2)));
    // on the handle's stream (ordered with the kernels that read the maps); `t` is a local: wait for the copy, on this stream only
    HIPCHK(hipMemcpyAsync(h->d_rect, t.data(), t.size() * sizeof(uint2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->rect_w = width; h->rect_h = height;
    return ORBX_OK;
}
// the digest alone, as orbx_set_rectification uploads it: pure host arithmetic, no handle, no device
extern "C" orbx_status orbx_debug_rect_digest(const float *map_x, const float *map_y, int64_t n, uint32_t *out_xy, uint32_t *out_frac) {
    if (n < 0 || (n > 0 && (!map_x || !map_y || !out_xy || !out_frac))) return orbx_fail(ORBX_BAD_ARGUMENT, "bad rectification maps");
    orbx_rect_digest(map_x, map_y, (size_t)n, out_xy, out_frac, 1);
    return ORBX_OK;
}
extern "C" orbx_status orbx_set_input_format(orbx_handle *h, int pixel_format) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "null handle");
    if (pixel_format < ORBX_FMT_GRAY8 || pixel_format > ORBX_FMT_BGRA8) return orbx_fail(ORBX_BAD_ARGUMENT, "unknown pixel format");
    if (h->d_rect && pixel_format != ORBX_FMT_GRAY8) return orbx_fail(ORBX_BAD_ARGUMENT, "rectification needs 8-bit gray input");
    h->input_format = pixel_format;
    return ORBX_OK;
}
static orbx_status run_chunk(orbx_handle *h, int B, const uint8_t *d_imgs, int W, int H, int stride,
                             int64_t frame_stride, orbx_keypoint *d_kps, uint8_t *d_desc, int32_t *d_counts,
                             int32_t *d_status, int cap, bool device_entry = false) {
    const DGeom &g = h->dg;
    // In-place level 0: only the device entry with grey, un-rectified, dword-aligned frames of at least ORBX_IP_MIN_W x
    // ORBX_IP_MIN_H pixels whose level-1 raw tap table passed the narrow check (geom.l1_inplace covers the last two); the fork
    // knob resizes level 1 on its own path.  Everything else runs k_pyr_l0 as before -- upstream handles included, whose geometry
    // carries no raw-coordinate tap table (geom.l1_inplace is false for them).
    const bool inplace = device_entry && h->l0_inplace && !h->l0_eager_sticky && !h->d_rect && h->input_format == ORBX_FMT_GRAY8 &&
                         h->p.pyramid_mode == ORBX_PYRAMID_FORK_PADDED && h->geom.l1_inplace && !h->resize_legacy && h->fork_level == 0 && ((uintptr_t)d_imgs & 3) == 0 &&
                         (stride & 3) == 0 && (frame_stride & 3) == 0 && frame_stride >= 0 && W == h->geom.width && H == h->geom.height;
    h->l0_pending = false;
    hipStream_t s = h->stream;
    const int NL = g.nlevels;
    if (h->d_rect && (h->rect_w != W || h->rect_h != H))
        return orbx_fail(ORBX_BAD_ARGUMENT, "rectification maps were set for another image size (raw and rectified size must agree)");
    // (no clearing launch: the per-frame status word is reset by the level-0 kernel, the per-level counters are written
    // unconditionally by k_quadtree)
    // (A two-stream level pipeline -- FAST of level l on a low-priority stream while the main stream resizes level
    // l+1 -- was measured and rejected: 81 k frames/s against 116 k for this single in-order sequence; the cross-stream
    // event waits and the 8 small FAST launches cost more than the overlap recovers.)
    //
    // Frames [f0, f0 + b) of the batch: every kernel takes its frame from the grid and indexes each per-frame buffer (input,
    // pyramid, status, candidate lists and counters, quadtree output, keypoints, descriptors) from a base pointer, so a
    // sub-batch is the same launch on offset base pointers.
    const int ngroups = (int)h->geom.fast_groups.size();
    // chain_only (the FAST-first plan): levels >= 1 alone -- no eager level-0 launch, and no status / cursor reset from level 1
    auto pyramid = [&](hipStream_t st, int f0, int b, int l_end, bool chain_only = false) {
        const uint8_t *im = d_imgs + (int64_t)f0 * frame_stride;
        uint8_t *pyr = h->d_pyr + (size_t)f0 * h->geom.pyr_bytes;
        int32_t *stp = d_status + f0;
        int *cc = h->d_cand_count + (size_t)f0 * NL;
        if (inplace) {   // no level-0 launch: level 1 reads the image and takes over the status / cursor reset
            { ProfScope ps(h, ORBX_K_PYR_RESIZE, st);
              const OrbxRaw0 raw = {im, (long long)frame_stride, W, H, stride};
              orbx_launch_pyr_resize_l1(st, g, b, h->d_taps + h->geom.l1_tap_begin, raw, pyr, h->geom.l1_tail_bx,
                                        chain_only ? nullptr : stp, chain_only ? nullptr : cc, h->rr_rpw); }
            for (int l = 2; l < l_end; ++l) {
                ProfScope ps(h, ORBX_K_PYR_RESIZE, st);
                orbx_launch_pyr_resize(st, g, b, l, h->d_taps, pyr, h->geom.lv[l].narrow_taps && !h->resize_legacy, h->rr_rpw);
            }
            return;
        }
        if (!chain_only) {
          ProfScope ps(h, ORBX_K_PYR_L0, st);
          if (h->d_rect) {   // cv::remap of the EuRoC rectification fused into level 0
              orbx_launch_pyr_l0_remap(st, g, b, im, W, H, stride, frame_stride, pyr, h->d_rect, stp, cc);
          } else if (h->input_format == ORBX_FMT_GRAY8) {
              orbx_launch_pyr_l0(st, g, b, im, W, H, stride, frame_stride, pyr, stp, cc);
          } else {   // cvtColor of Tracking::GrabImage* fused into level 0
              const int nch = (h->input_format == ORBX_FMT_RGB8 || h->input_format == ORBX_FMT_BGR8) ? 3 : 4;
              const bool rgb = h->input_format == ORBX_FMT_RGB8 || h->input_format == ORBX_FMT_RGBA8;
              orbx_launch_pyr_l0_color(st, g, b, im, W, H, stride, frame_stride, pyr, nch, rgb ? 0 : 2, rgb ? 2 : 0, stp, cc);
          } }
        for (int l = 1; l < l_end; ++l) {
            ProfScope ps(h, ORBX_K_PYR_RESIZE, st);
            orbx_launch_pyr_resize(st, g, b, l, h->d_taps, pyr, h->geom.lv[l].narrow_taps && !h->resize_legacy, h->rr_rpw);
        }
    };
    // part: 0 = any groups (mixed kernel when in place), 1 = level-0 groups only, 2 = groups of levels >= 1 only (the two launches
    // of the FAST-first plan: each sized from its own tallest cell, the second never in place)
    auto fast = [&](hipStream_t st, int f0, int b, int g0, int ng, int lds_floor, int part = 0) {
        ProfScope ps(h, ORBX_K_FAST, st);
        const OrbxRaw0 raw = {d_imgs + (int64_t)f0 * frame_stride, (long long)frame_stride, W, H, stride};
        orbx_launch_fast_rows(st, g, b, h->d_cells, h->d_groups + g0, ng, h->d_pyr + (size_t)f0 * h->geom.pyr_bytes,
                              h->d_dense + (size_t)f0 * g.cand_total, h->d_cand_count + (size_t)f0 * NL, d_status + f0,
                              part == 1 ? h->max_ch_l0 : part == 2 ? h->max_ch_rest : h->max_ch,
                              h->fast_lcap, h->fast_stop, lds_floor, inplace && part != 2 ? &raw : nullptr, part == 1,
                              h->fast_gpw);
    };
    auto finish = [&](int f0, int b) {
        { ProfScope ps(h, ORBX_K_QUADTREE);
          orbx_launch_quadtree(s, g, b, h->d_dense + (size_t)f0 * g.cand_total, h->d_cand_count + (size_t)f0 * NL,
                               h->d_lvl_kp + (size_t)f0 * g.kp_total, h->d_lvl_count + (size_t)f0 * NL, d_status + f0,
                               h->d_knode + (size_t)f0 * g.cand_total, h->ncap, (long long)b * NL >= 1024 ? h->lds_keys : h->lds_keys_few, h->qt_reg_keys, 0, NL); }
        // orientation (IC_Angle) is computed inside k_describe from the same LDS patch the descriptor uses
        { ProfScope ps(h, ORBX_K_DESC);
          const OrbxRaw0 raw = {d_imgs + (int64_t)f0 * frame_stride, (long long)frame_stride, W, H, stride};
          orbx_launch_describe(s, g, b, h->d_pyr + (size_t)f0 * h->geom.pyr_bytes, h->d_lvl_kp + (size_t)f0 * g.kp_total,
                               h->d_lvl_count + (size_t)f0 * NL, h->d_lvl_angle + (size_t)f0 * g.kp_total, d_kps + (int64_t)f0 * cap,
                               d_desc + (int64_t)f0 * cap * 32, d_counts + f0, d_status + f0, cap, inplace ? &raw : nullptr); }
    };
    h->blur_valid = false;  // the Gaussian is fused into k_describe; the full blurred image is only built on request
    if (inplace) {          // what ensure_level0() would build the slab's level 0 of this batch from
        h->l0_src = OrbxRaw0{d_imgs, (long long)frame_stride, W, H, stride};
        h->l0_pending = true;
    }
    // Sub-batch pipeline (large batches): the pyramids of the S sub-batches are queued on the high-priority side stream, FAST ->
    // quadtree -> descriptors of sub-batch k on the main stream once the pyramid of k is done.  The pyramid is bound by load
    // latency (its waves leave most of a CU's vector port idle), FAST and the descriptors by vector issue: pyramid k+1 takes
    // the wave slots the main stream's kernels free while they work on sub-batch k (73-87 % of the pyramid's time overlaps
    // them, but the kernels slow each other: about 2 % per step, profiles/r04_pipeline.md).  The first sub-batch is the
    // small one by default: its pyramid is the only one nothing hides.  The calibration pass that profiles every kernel
    // (more than one bit of the profiling mask) runs the serial sequence below, so that each kernel's time is its own; a
    // single-kernel profile keeps the pipeline and times each of the S launches of that kernel from its stream, which includes
    // the time it shares the CUs with the other stream's kernels.
    //
    // FAST-first plan (the default of large batches): the level-0 FAST groups need no pyramid level this
    // call builds on the side stream -- in place they read the caller's image, otherwise the padded level 0 the main stream has just
    // written -- so FAST starts at once and all of FAST is the window the resize chains of the sub-batches run under; the FAST
    // groups of levels >= 1 follow per sub-batch as its chain completes.  Quadtree and descriptors run once over the batch, after
    // the last chain: the pyramid shares the CUs with FAST only (the kernel it slows least, profiles/r04_pipeline.md).  A late
    // chain makes the main stream wait and then runs alone, so the plan is never much worse than the serial sequence.  Level 1's
    // in-place launch would reset status / cursors beside the level-0 FAST groups that update them: one k_clear does it up front.
    if (h->fast_first && B >= h->plan_min_frames && __builtin_popcount(h->prof_mask) <= 1) {
        int off[ORBX_PIPE_MAX + 1];
        const int n = orbx_split_batch(B, h->plan_sub, h->plan_head, off);
        const int ng0 = h->l0_groups;
        hipStream_t s2 = h->plan_stream;
        if (inplace) {
            ProfScope ps(h, ORBX_K_MISC);
            orbx_launch_clear(s, d_status, B, h->d_cand_count, B * NL, nullptr, 0);
        } else {
            pyramid(s, 0, B, 1);   // the eager level 0 of the whole batch (resets status and cursors itself)
        }
        if (hipEventRecord(h->ev_fork, s) != hipSuccess || hipStreamWaitEvent(s2, h->ev_fork, 0) != hipSuccess)
            { hipStreamSynchronize(s2); return orbx_fail(ORBX_HIP_ERROR, "plan fork event"); }
        for (int k = 0; k < n; ++k) {
            pyramid(s2, off[k], off[k + 1] - off[k], NL, true);
            if (hipEventRecord(h->ev_pipe[k], s2) != hipSuccess)
                { hipStreamSynchronize(s2); return orbx_fail(ORBX_HIP_ERROR, "plan event"); }
        }
        fast(s, 0, B, 0, ng0, 0, 1);
        for (int k = 0; k < n; ++k) {
            if (hipStreamWaitEvent(s, h->ev_pipe[k], 0) != hipSuccess)
                { hipStreamSynchronize(s2); return orbx_fail(ORBX_HIP_ERROR, "plan event wait"); }
            fast(s, off[k], off[k + 1] - off[k], ng0, ngroups - ng0, 0, 2);
        }
        finish(0, B);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { hipStreamSynchronize(s2); return orbx_fail(ORBX_HIP_ERROR, std::string("kernel launch: ") + hipGetErrorString(e)); }
        h->last_batch = B;
        return ORBX_OK;
    }
    if (h->pipeline > 1 && B >= ORBX_PIPE_MIN_FRAMES && __builtin_popcount(h->prof_mask) <= 1) {
        int off[ORBX_PIPE_MAX + 1];
        const int S = orbx_split_batch(B, h->pipeline, h->pipe_head, off);   // = h->pipeline: B >= ORBX_PIPE_MIN_FRAMES
        hipStream_t s2 = h->side_stream;
        // the side stream starts behind everything queued on the main stream so far (the frames' upload, the previous batch's
        // readers of the pyramid and of the outputs); every sub-batch's FAST launch waits for its pyramid, and the last of those
        // waits joins the side stream.  Any error exit waits for the side stream: its work reads and writes the handle's buffers.
        if (hipEventRecord(h->ev_fork, s) != hipSuccess || hipStreamWaitEvent(s2, h->ev_fork, 0) != hipSuccess)
            { hipStreamSynchronize(s2); return orbx_fail(ORBX_HIP_ERROR, "pipeline fork event"); }
        for (int k = 0; k < S; ++k) {
            pyramid(s2, off[k], off[k + 1] - off[k], NL);
            if (hipEventRecord(h->ev_pipe[k], s2) != hipSuccess)
                { hipStreamSynchronize(s2); return orbx_fail(ORBX_HIP_ERROR, "pipeline event"); }
        }
        const int floor = h->fast_room ? ORBX_LDS_PER_CU / ORBX_FAST_PIPE_WAVES : 0;
        for (int k = 0; k < S; ++k) {
            if (hipStreamWaitEvent(s, h->ev_pipe[k], 0) != hipSuccess)
                { hipStreamSynchronize(s2); return orbx_fail(ORBX_HIP_ERROR, "pipeline event wait"); }
            fast(s, off[k], off[k + 1] - off[k], 0, ngroups, floor);
            finish(off[k], off[k + 1] - off[k]);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { hipStreamSynchronize(s2); return orbx_fail(ORBX_HIP_ERROR, std::string("kernel launch: ") + hipGetErrorString(e)); }
        h->last_batch = B;
        return ORBX_OK;
    }
    // Large batches fork after level fork_level - 1: the remaining (small) levels are resized on the high-priority side stream
    // -- seven dependent launches of which the last four have few waves and are pure latency -- followed by their FAST
    // groups, while the main stream runs the issue-bound FAST kernel of the large levels; joined before the quadtree.
    const bool fork = h->fork_level > 0 && (long long)B * ngroups >= 16384;
    pyramid(s, 0, B, fork ? h->fork_level : NL);
    if (fork) {
        hipStream_t s2 = h->side_stream;
        if (hipEventRecord(h->ev_fork, s) != hipSuccess || hipStreamWaitEvent(s2, h->ev_fork, 0) != hipSuccess)
            return orbx_fail(ORBX_HIP_ERROR, "fork event");
        for (int l = h->fork_level; l < NL; ++l) {
            ProfScope ps(h, ORBX_K_PYR_RESIZE, s2);
            orbx_launch_pyr_resize(s2, g, B, l, h->d_taps, h->d_pyr, h->geom.lv[l].narrow_taps && !h->resize_legacy, h->rr_rpw);
        }
        fast(s2, 0, B, h->fork_group, ngroups - h->fork_group, 0);
        // (The quadtree of the small levels was tried on the side stream behind its FAST groups: it needs CU residency the
        // FAST kernel of the large levels does not give up -- 201 us for 1024 workgroups that take 57 us alone -- and delays the
        // join.  It runs after the join.)
        fast(s, 0, B, 0, h->fork_group, 0);
        if (hipEventRecord(h->ev_join, s2) != hipSuccess || hipStreamWaitEvent(s, h->ev_join, 0) != hipSuccess)
            { hipStreamSynchronize(s2); return orbx_fail(ORBX_HIP_ERROR, "join event"); }   // the side stream's work reads the handle's buffers: never leave it unjoined
    } else if (h->fast_first && B >= h->plan_min_frames) {
        // the calibration pass of a batch the FAST-first plan would take (more than one bit of the profiling mask): the plan's
        // two FAST kernels, one after the other and alone on the chip, so that the k_fast_rows slot is theirs
        fast(s, 0, B, 0, h->l0_groups, 0, 1);
        fast(s, 0, B, h->l0_groups, ngroups - h->l0_groups, 0, 2);
    } else {
        fast(s, 0, B, 0, ngroups, 0);
    }
    finish(0, B);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, std::string("kernel launch: ") + hipGetErrorString(e));
    h->last_batch = B;
    return ORBX_OK;
}

extern "C" orbx_status orbx_extract_batch_device(orbx_handle *h, int nframes, const uint8_t *d_imgs, int width,
                                                 int height, int stride, int64_t frame_stride, orbx_keypoint *d_kps,
                                                 uint8_t *d_desc, int32_t *d_counts, int32_t *d_status, int cap) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "null handle");
    if (!d_imgs || width <= 0 || height <= 0 || nframes <= 0) return orbx_fail(ORBX_EMPTY_IMAGE, "empty image");
    if (!d_kps || !d_desc || !d_counts || cap <= 0 || stride < width * orbx_fmt_channels(h->input_format)) return orbx_fail(ORBX_BAD_ARGUMENT, "bad output buffers / stride");
    orbx_status st = configure(h, width, height);
    if (st != ORBX_OK) return st;
    HIPCHK(hipSetDevice(h->dev));
    const int MB = h->p.max_batch;
    for (int f0 = 0; f0 < nframes; f0 += MB) {
        const int B = std::min(MB, nframes - f0);
        int32_t *stp = d_status ? d_status + f0 : h->d_status;
        st = run_chunk(h, B, d_imgs + (int64_t)f0 * frame_stride, width, height, stride, frame_stride,
                       d_kps + (int64_t)f0 * cap, d_desc + (int64_t)f0 * cap * 32, d_counts + f0, stp, cap, true);
        if (st != ORBX_OK) return st;
    }
    return ORBX_OK;
}

// Host-buffer entry point: two sets of device staging buffers and two copy streams, so that the upload of chunk c+1 and
// the download of chunk c-1 overlap the kernels of chunk c.  With pageable host memory hipMemcpyAsync stages through the
// runtime's pinned buffers and blocks the calling thread while it does (the GPU keeps computing meanwhile); with pinned
// memory (orbx_host_alloc, or any hipHostMalloc / hipHostRegister memory) every copy is a plain asynchronous DMA.
static orbx_status ensure_staging(orbx_handle *h, size_t in_bytes, int cap, int chunk) {
    if (in_bytes > h->d_in_bytes || cap > h->out_cap || chunk > h->stage_chunk) {
        HIPCHK(hipStreamSynchronize(h->stream));
        const size_t inb = std::max(in_bytes, h->d_in_bytes);
        const int c = std::max(cap, h->out_cap), ch = std::max(chunk, h->stage_chunk);
        for (int s = 0; s < 2; ++s) {
            hipFree(h->st_in[s]); hipFree(h->st_kps[s]);   // st_desc / st_cnt live inside the st_kps allocation
            h->st_in[s] = nullptr; h->st_kps[s] = nullptr; h->st_desc[s] = nullptr; h->st_cnt[s] = nullptr;
        }
        h->d_in_bytes = 0; h->out_cap = 0; h->stage_chunk = 0;
        for (int s = 0; s < 2; ++s) {
            HIPCHK(hipMalloc(&h->st_in[s], inb));
            // one block per set: keypoints | descriptors | counts | status -- a call that fills the block exactly (the
            // single-frame drop-in call) downloads it with ONE copy
            const size_t kb = (size_t)ch * c * sizeof(orbx_keypoint), db = (size_t)ch * c * 32;
            uint8_t *blk = nullptr;
            HIPCHK(hipMalloc(&blk, kb + db + (size_t)2 * ch * sizeof(int)));
            h->st_kps[s] = (orbx_keypoint *)blk; h->st_desc[s] = blk + kb; h->st_cnt[s] = (int *)(blk + kb + db);
        }
        h->d_in_bytes = inb; h->out_cap = c; h->stage_chunk = ch;
    }
    if (!h->s_in) {
        // the copy stream gets the high priority level: the runtime maps streams of one priority onto a small shared pool of
        // hardware queues (4 by default), and a copy stream that lands on the compute stream's queue serialises uploads with
        // the kernels (measured: 95 k instead of 153 k frames/s in a process that had created a few streams before the handle)
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&h->s_in, hipStreamNonBlocking, hi));
        for (int s = 0; s < 2; ++s) {
            HIPCHK(hipEventCreateWithFlags(&h->ev_in[s], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&h->ev_done[s], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&h->ev_out[s], hipEventDisableTiming));
        }
    }
    return ORBX_OK;
}

extern "C" void *orbx_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
extern "C" void orbx_host_free(void *p) { if (p) hipHostFree(p); }

// The RGB-D part of orbx_extract_rgbd_batch (NULL for orbx_extract_batch): k_rgbd runs behind every chunk's kernels on the
// chunk's keypoints, reading the chunk's depth from staging or, mapped, from the caller's memory.
struct RgbdHost {
    const uint8_t *depth; int format, stride; int64_t frame_stride; float scale, mbf; int scale_f32;
    double K4[4], k14[14]; int identity;
    orbx_keypoint *kps_un; float *u_right, *depth_out;
};
static int depth_elem(int format) { return format == ORBX_DEPTH_U16 ? 2 : 4; }
// bytes of one depth frame the kernel may read: (H - 1) rows and the W samples of the last one
static int64_t depth_span(int format, int width, int height, int stride) {
    return (int64_t)(height - 1) * stride + (int64_t)width * depth_elem(format);
}
static orbx_status ensure_rgbd_staging(orbx_handle *h, size_t dep_bytes, size_t rg_bytes) {
    if (dep_bytes <= h->dep_bytes && rg_bytes <= h->rg_bytes) return ORBX_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t db = std::max(dep_bytes, h->dep_bytes), rb = std::max(rg_bytes, h->rg_bytes);
    for (int s = 0; s < 2; ++s) { hipFree(h->st_dep[s]); hipFree(h->st_rg[s]); h->st_dep[s] = nullptr; h->st_rg[s] = nullptr; }
    h->dep_bytes = 0; h->rg_bytes = 0;
    for (int s = 0; s < 2; ++s) {
        if (db) HIPCHK(hipMalloc(&h->st_dep[s], db));
        HIPCHK(hipMalloc(&h->st_rg[s], rb));
    }
    h->dep_bytes = db; h->rg_bytes = rb;
    return ORBX_OK;
}

static orbx_status extract_host(orbx_handle *h, int nframes, const uint8_t *imgs, int width, int height, int stride,
                                int64_t frame_stride, orbx_keypoint *kps, uint8_t *desc, int32_t *counts, int cap,
                                const RgbdHost *rg) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "null handle");
    if (!imgs || width <= 0 || height <= 0 || nframes <= 0) return orbx_fail(ORBX_EMPTY_IMAGE, "empty image");
    if (!kps || !desc || !counts || cap <= 0 || stride < width * orbx_fmt_channels(h->input_format)) return orbx_fail(ORBX_BAD_ARGUMENT, "bad output buffers / stride");
    orbx_status st = configure(h, width, height);
    if (st != ORBX_OK) return st;
    HIPCHK(hipSetDevice(h->dev));
    const int MB = h->p.max_batch;
    // chunks of max_batch frames (all frames of a call that fits one chunk stay resident for the pyramid accessors);
    // longer calls are pipelined chunk by chunk
    const int chunk = std::min(MB, nframes);
    const size_t fbytes = (size_t)stride * height;
    st = ensure_staging(h, (size_t)chunk * fbytes, cap, chunk);
    if (st != ORBX_OK) return st;
    const int nchunks = (nframes + chunk - 1) / chunk;
    // counts | status of every chunk of the call land here (page-locked: a pageable landing place would make each copy
    // synchronous), one slot per chunk so that nothing is reused before the call's single final wait
    if ((size_t)2 * nchunks * chunk > h->pin_stat_ints) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->s_in) HIPCHK(hipStreamSynchronize(h->s_in));
        if (h->pin_stat) { hipHostFree(h->pin_stat); h->pin_stat = nullptr; h->pin_stat_ints = 0; }
        HIPCHK(hipHostMalloc((void **)&h->pin_stat, (size_t)2 * nchunks * chunk * sizeof(int), hipHostMallocDefault));
        h->pin_stat_ints = (size_t)2 * nchunks * chunk;
    }
    int *hstat = h->pin_stat;
    orbx_status worst = ORBX_OK;
    // RGB-D depth: read in place over the link when the caller's depth is page-locked and device-mapped (about one 64-byte
    // sample per keypoint instead of the whole frame) unless ORBX_RGBD_DEPTH=upload; staged chunk by chunk otherwise, dfb bytes
    // per frame in staging
    const uint8_t *d_inplace = nullptr;
    const int64_t dspan = rg ? depth_span(rg->format, width, height, rg->stride) : 0, dfb = rg ? (int64_t)rg->stride * height : 0;
    if (rg) {
        const char *e = getenv("ORBX_RGBD_DEPTH");
        const bool want_inplace = e ? strcmp(e, "inplace") == 0 : ORBX_RGBD_INPLACE_DEFAULT;
        void *pd = nullptr;
        if (want_inplace && hipHostGetDevicePointer(&pd, (void *)rg->depth, 0) == hipSuccess && pd) d_inplace = (const uint8_t *)pd;
        else (void)hipGetLastError();
        st = ensure_rgbd_staging(h, d_inplace ? 0 : (size_t)chunk * dfb, (size_t)chunk * cap * (sizeof(orbx_keypoint) + 2 * sizeof(float)));
        if (st != ORBX_OK) return st;
    }
    // a single chunk needs no second stream: copies and kernels in order on the handle's stream (the latency path)
    const bool piped = nchunks > 1;
    // Pipelined calls use ONE copy stream for both directions: upload(c+1) and download(c-1) take turns on it while chunk c
    // computes.  (Round 2 had a second stream for the downloads; with uploads, downloads and kernels all in flight at once the
    // kernels of chunks >= 1 ran 1.4-5x slower from page-locked caller memory -- profiles/r03_host_io_trace.txt -- and
    // page-locked memory lost to pageable memory: 88 k against 103 k frames/s.  With one copy stream, the download queued in
    // front of the next upload and every dependency a stream-side event wait, the copy stream is busy back to back.)
    hipStream_t sin = piped ? h->s_in : h->stream, sout = sin;
    auto upload = [&](int c) -> hipError_t {
        const int s = c & 1, f0 = c * chunk, B = std::min(chunk, nframes - f0);
        if (c >= 2) {   // the kernels of chunk c-2 read this input set
            const hipError_t e = hipStreamWaitEvent(sin, h->ev_done[s], 0);
            if (e != hipSuccess) return e;
        }
        if (frame_stride == (int64_t)fbytes) {   // frames back to back: one copy per chunk
            const hipError_t e = hipMemcpyAsync(h->st_in[s], imgs + (int64_t)f0 * frame_stride, (size_t)B * fbytes, hipMemcpyHostToDevice, sin);
            if (e != hipSuccess) return e;
        } else {
            for (int i = 0; i < B; ++i) {
                const hipError_t e = hipMemcpyAsync(h->st_in[s] + (size_t)i * fbytes, imgs + (int64_t)(f0 + i) * frame_stride, fbytes,
                                                    hipMemcpyHostToDevice, sin);
                if (e != hipSuccess) return e;
            }
        }
        if (rg && !d_inplace) {   // the chunk's depth frames, dfb bytes apart in staging: only the span the kernel may read
            if (rg->frame_stride == dfb) {
                const hipError_t e = hipMemcpyAsync(h->st_dep[s], rg->depth + (int64_t)f0 * dfb, (size_t)((B - 1) * dfb + dspan),
                                                    hipMemcpyHostToDevice, sin);
                if (e != hipSuccess) return e;
            } else {
                for (int i = 0; i < B; ++i) {
                    const hipError_t e = hipMemcpyAsync(h->st_dep[s] + (int64_t)i * dfb, rg->depth + (int64_t)(f0 + i) * rg->frame_stride,
                                                        (size_t)dspan, hipMemcpyHostToDevice, sin);
                    if (e != hipSuccess) return e;
                }
            }
        }
        return piped ? hipEventRecord(h->ev_in[s], sin) : hipSuccess;
    };
    // Page-locked, device-mapped output buffers (orbx_host_alloc, hipHostMalloc, hipHostRegister with the mapped flag) are
    // written by k_describe ITSELF over the link: the results leave while the chunk computes and while the next chunk's frames
    // come in on the link's other direction, and the copy stream carries uploads only (134 k against 120 k frames/s at chunks
    // of 64, 256 frames per call).  Only the per-frame counts | status stay in device memory (several kernels update the
    // status with atomics) and come back with one small copy per chunk.  The caller reads its buffers after the call returns
    // (the call ends with a wait on both streams), as with the copies.
    orbx_keypoint *zk = nullptr; uint8_t *zd = nullptr;
    {
        void *pk = nullptr, *pd = nullptr;
        if (hipHostGetDevicePointer(&pk, kps, 0) == hipSuccess && hipHostGetDevicePointer(&pd, desc, 0) == hipSuccess && pk && pd) {
            zk = (orbx_keypoint *)pk; zd = (uint8_t *)pd;
        } else {
            (void)hipGetLastError();   // pageable (or unmapped) buffers: results are staged in device memory and copied
        }
    }
    // RGB-D outputs: written in place when all three are mapped (as kps / desc above), staged otherwise
    orbx_keypoint *zun = nullptr; float *zur = nullptr, *zdp = nullptr;
    if (rg) {
        void *pu = nullptr, *pr = nullptr, *pd = nullptr;
        if (hipHostGetDevicePointer(&pu, rg->kps_un, 0) == hipSuccess && hipHostGetDevicePointer(&pr, rg->u_right, 0) == hipSuccess &&
            hipHostGetDevicePointer(&pd, rg->depth_out, 0) == hipSuccess && pu && pr && pd) {
            zun = (orbx_keypoint *)pu; zur = (float *)pr; zdp = (float *)pd;
        } else {
            (void)hipGetLastError();
        }
    }
    // download of chunk c: queued behind the chunk's kernels; its event frees the output set for chunk c+2's kernels
    auto download_enqueue = [&](int c) -> hipError_t {
        const int s = c & 1, f0 = c * chunk, B = std::min(chunk, nframes - f0);
        hipError_t e = piped ? hipStreamWaitEvent(sout, h->ev_done[s], 0) : hipSuccess;
        if (e == hipSuccess && !zk) e = hipMemcpyAsync(kps + (int64_t)f0 * cap, h->st_kps[s], (size_t)B * cap * sizeof(orbx_keypoint), hipMemcpyDeviceToHost, sout);
        if (e == hipSuccess && !zk) e = hipMemcpyAsync(desc + (int64_t)f0 * cap * 32, h->st_desc[s], (size_t)B * cap * 32, hipMemcpyDeviceToHost, sout);
        if (rg && !zun) {
            const size_t nk = (size_t)chunk * cap;
            if (e == hipSuccess) e = hipMemcpyAsync(rg->kps_un + (int64_t)f0 * cap, h->st_rg[s], (size_t)B * cap * sizeof(orbx_keypoint), hipMemcpyDeviceToHost, sout);
            if (e == hipSuccess) e = hipMemcpyAsync(rg->u_right + (int64_t)f0 * cap, h->st_rg[s] + nk * sizeof(orbx_keypoint), (size_t)B * cap * sizeof(float), hipMemcpyDeviceToHost, sout);
            if (e == hipSuccess) e = hipMemcpyAsync(rg->depth_out + (int64_t)f0 * cap, h->st_rg[s] + nk * (sizeof(orbx_keypoint) + sizeof(float)), (size_t)B * cap * sizeof(float), hipMemcpyDeviceToHost, sout);
        }
        // counts | status are one device block (st_cnt[s][0 .. 2 chunk)): ONE small copy (every copy costs ~15 us of link
        // turn-around whatever its size); the counts go on to the caller's array from the landing buffer
        if (e == hipSuccess) e = hipMemcpyAsync(hstat + (size_t)c * 2 * chunk, h->st_cnt[s], (size_t)2 * chunk * sizeof(int), hipMemcpyDeviceToHost, sout);
        if (e == hipSuccess && piped) e = hipEventRecord(h->ev_out[s], sout);
        return e;
    };
    auto collect = [&]() {   // after the final wait: counts to the caller, worst status of the call
        for (int c = 0; c < nchunks; ++c) {
            const int f0 = c * chunk, B = std::min(chunk, nframes - f0);
            for (int i = 0; i < B; ++i) {
                counts[f0 + i] = hstat[(size_t)c * 2 * chunk + i];
                if (hstat[(size_t)c * 2 * chunk + chunk + i] != ORBX_OK) worst = (orbx_status)hstat[(size_t)c * 2 * chunk + chunk + i];
            }
        }
    };
    // Every error exit from here on waits for both streams first: kernels and copies may still be writing the caller's
    // buffers (zero-copy outputs) or reading them (in-place depth), and the caller may free them once the call returns.
#define DRAINCHK(expr)                                                                                              \
    do {                                                                                                            \
        hipError_t _e = (expr);                                                                                     \
        if (_e != hipSuccess) {                                                                                     \
            hipStreamSynchronize(h->stream); hipStreamSynchronize(sin);                                             \
            return orbx_fail(ORBX_HIP_ERROR, std::string(#expr) + ": " + hipGetErrorString(_e));                         \
        }                                                                                                           \
    } while (0)
    // Latency path (one chunk that fills its staging block exactly, a few MB at most -- the drop-in call of Tracking.cc): the
    // frames go through page-locked staging (one true DMA instead of a runtime-staged pageable copy) and the results come
    // back with ONE copy of the whole output block instead of four.
    const size_t out_bytes = (size_t)chunk * cap * (sizeof(orbx_keypoint) + 32) + (size_t)2 * chunk * sizeof(int);
    const size_t in_bytes_q = (size_t)nframes * fbytes;
    const bool stage_in = in_bytes_q <= ((size_t)1 << 20);   // beyond ~1 MB the host-side memcpy costs more than the runtime's own staging
    const bool quick = !rg && !piped && nframes == h->stage_chunk && cap == h->out_cap && out_bytes <= ((size_t)4 << 20) &&
                       stage_pin(h, (stage_in ? in_bytes_q : 0) + out_bytes) == ORBX_OK;
    if (quick) {
        uint8_t *pin_in = h->pin, *pin_out = h->pin + (stage_in ? in_bytes_q : 0);
        if (stage_in) {
            for (int i = 0; i < nframes; ++i) memcpy(pin_in + (size_t)i * fbytes, imgs + (int64_t)i * frame_stride, fbytes);
            DRAINCHK(hipMemcpyAsync(h->st_in[0], pin_in, in_bytes_q, hipMemcpyHostToDevice, h->stream));
        } else {
            DRAINCHK(upload(0));
        }
        st = run_chunk(h, nframes, h->st_in[0], width, height, stride, (int64_t)fbytes, h->st_kps[0], h->st_desc[0], h->st_cnt[0],
                       h->st_cnt[0] + chunk, cap);
        if (st != ORBX_OK) { hipStreamSynchronize(h->stream); return st; }
        DRAINCHK(hipMemcpyAsync(pin_out, h->st_kps[0], out_bytes, hipMemcpyDeviceToHost, h->stream));
        DRAINCHK(hipStreamSynchronize(h->stream));
        const size_t kb = (size_t)nframes * cap * sizeof(orbx_keypoint), db = (size_t)nframes * cap * 32;
        const int *cnt = (const int *)(pin_out + kb + db);
        // only the meaningful part of every frame's records leaves the staging buffer
        for (int i = 0; i < nframes; ++i) {
            const int n = std::min(std::max(cnt[i], 0), cap);
            memcpy(kps + (int64_t)i * cap, pin_out + (size_t)i * cap * sizeof(orbx_keypoint), (size_t)n * sizeof(orbx_keypoint));
            memcpy(desc + (int64_t)i * cap * 32, pin_out + kb + (size_t)i * cap * 32, (size_t)n * 32);
            counts[i] = cnt[i];
            if (cnt[nframes + i] != ORBX_OK) worst = (orbx_status)cnt[nframes + i];
        }
        if (worst != ORBX_OK) return orbx_fail(worst, "a frame exceeded the keypoint / candidate capacity");
        return ORBX_OK;
    }
    DRAINCHK(upload(0));
    for (int c = 0; c < nchunks; ++c) {
        const int s = c & 1, f0 = c * chunk, B = std::min(chunk, nframes - f0);
        if (piped) DRAINCHK(hipStreamWaitEvent(h->stream, h->ev_in[s], 0));             // the chunk's frames have arrived
        orbx_keypoint *ck = zk ? zk + (int64_t)f0 * cap : h->st_kps[s];
        st = run_chunk(h, B, h->st_in[s], width, height, stride, (int64_t)fbytes, ck, zk ? zd + (int64_t)f0 * cap * 32 : h->st_desc[s],
                       h->st_cnt[s], h->st_cnt[s] + chunk, cap);
        if (st != ORBX_OK) { hipStreamSynchronize(h->stream); hipStreamSynchronize(sin); return st; }
        if (rg) {   // Frame::ComputeStereoFromRGBD behind the chunk's kernels, on the records they just wrote
            const size_t nk = (size_t)chunk * cap;
            OrbxRgbdArgs a;
            a.depth = d_inplace ? d_inplace + (int64_t)f0 * rg->frame_stride : h->st_dep[s];
            a.frame_stride = d_inplace ? rg->frame_stride : dfb; a.stride = rg->stride;
            a.format = rg->format; a.width = width; a.height = height; a.scale_f32 = rg->scale_f32; a.scale = rg->scale; a.mbf = rg->mbf;
            { ProfScope ps(h, ORBX_K_MISC);
              orbx_launch_rgbd(h->stream, B, cap, cap, rg->K4, rg->k14, rg->identity, a, ck, nullptr, h->st_cnt[s],
                               zun ? zun + (int64_t)f0 * cap : (orbx_keypoint *)h->st_rg[s],
                               zun ? zur + (int64_t)f0 * cap : (float *)(h->st_rg[s] + nk * sizeof(orbx_keypoint)),
                               zun ? zdp + (int64_t)f0 * cap : (float *)(h->st_rg[s] + nk * (sizeof(orbx_keypoint) + sizeof(float)))); }
            DRAINCHK(hipGetLastError());
        }
        if (piped) DRAINCHK(hipEventRecord(h->ev_done[s], h->stream));
        // copy stream: results of chunk c-1 first (its kernels are done or nearly so), then the frames of chunk c+1 (its input
        // set was read by chunk c-1: the download in front of it already waited for that chunk)
        if (c >= 1) DRAINCHK(download_enqueue(c - 1));
        if (c + 1 < nchunks) DRAINCHK(upload(c + 1));
        // the calling thread stays one chunk ahead of the device, not more: it waits here until chunk c-1's results have left
        // their output set, which chunk c+1's kernels (enqueued next) write.  (Letting it run ahead of the whole call with
        // stream-side waits instead was measured: 82 k against 111 k frames/s at chunks of 32, 84 k against 95 k at 16 chunks
        // of 64 -- many queued cross-stream waits cost more than the wake-ups they save.)
        if (piped && c >= 1) DRAINCHK(hipEventSynchronize(h->ev_out[(c - 1) & 1]));
    }
    DRAINCHK(download_enqueue(nchunks - 1));
    DRAINCHK(hipStreamSynchronize(sout));
    if (piped) DRAINCHK(hipStreamSynchronize(h->stream));
#undef DRAINCHK
    collect();
    if (worst != ORBX_OK) return orbx_fail(worst, "a frame exceeded the keypoint / candidate capacity");
    return ORBX_OK;
}

extern "C" orbx_status orbx_extract_batch(orbx_handle *h, int nframes, const uint8_t *imgs, int width, int height,
                                          int stride, int64_t frame_stride, orbx_keypoint *kps, uint8_t *desc,
                                          int32_t *counts, int cap) {
    return extract_host(h, nframes, imgs, width, height, stride, frame_stride, kps, desc, counts, cap, nullptr);
}

// ---------------------------------------------------------------- RGB-D Frame: Frame::ComputeStereoFromRGBD (k_rgbd)
// camera4 / dist as the doubles k_undistort and k_rgbd take (section (f)2 below); dist[0] == 0: identity.  The ONE copy of the
// coefficient rule: k_undistort evaluates k[0..11] (radial, tangential, rational, thin prism); the tilted-sensor terms tauX,
// tauY (dist[12], dist[13]) are not implemented, so a model that sets either is refused instead of being answered without them.
static orbx_status undistort_args(const float *camera4, const float *dist, int ndist, double *K4, double *k14, int *identity) {
    for (int i = 12; i < ndist && i < 14; ++i)
        if (dist[i] != 0.0f)   // (NaN included)
            return orbx_fail(ORBX_UNSUPPORTED, "the tilt terms of the distortion model (dist[12], dist[13]: tauX, tauY) are not supported; at most 12 coefficients are evaluated");
    if (!camera4) { *identity = 1; return ORBX_OK; }   // (orbx_image_bounds asking for the rule alone)
    for (int i = 0; i < 4; ++i) K4[i] = (double)camera4[i];
    for (int i = 0; i < 14; ++i) k14[i] = i < ndist ? (double)dist[i] : 0.0;
    *identity = (ndist < 1 || dist[0] == 0.0f) ? 1 : 0;
    return ORBX_OK;
}
// argument rules shared by the three RGB-D entry points (checked before any device work)
static orbx_status rgbd_check(int nframes, const void *depth, int format, int width, int height, int stride, int64_t frame_stride) {
    if (format != ORBX_DEPTH_U16 && format != ORBX_DEPTH_F32) return orbx_fail(ORBX_BAD_ARGUMENT, "unknown depth format");
    const int el = depth_elem(format);
    if (!depth || width <= 0 || height <= 0) return orbx_fail(ORBX_BAD_ARGUMENT, "empty depth image");
    if ((int64_t)stride < (int64_t)width * el || stride % el != 0) return orbx_fail(ORBX_BAD_ARGUMENT, "depth stride below W * element size or not a multiple of it");
    if ((uintptr_t)depth % el != 0) return orbx_fail(ORBX_BAD_ARGUMENT, "depth pointer not aligned to its element size");
    if (nframes > 1 && (frame_stride % el != 0 || frame_stride < depth_span(format, width, height, stride)))
        return orbx_fail(ORBX_BAD_ARGUMENT, "depth frame stride overlaps the frames or is not a multiple of the element size");
    return ORBX_OK;
}
// mDepthMapFactor != 1 (|f - 1| > 1e-5, src/Tracking.cc:327): f32 input is converted in place; u16 input always is
static int rgbd_scale_f32(int format, float scale) { return format == ORBX_DEPTH_F32 && (double)fabsf(scale - 1.0f) > 1e-5; }

extern "C" orbx_status orbx_rgbd_depth_device(orbx_handle *h, int nframes, const orbx_keypoint *d_kps, const int32_t *d_counts, int cap,
                                              const float *camera4, const float *dist, int ndist, const void *d_depth, int depth_format,
                                              int width, int height, int stride, int64_t frame_stride, float depth_scale, float mbf,
                                              orbx_keypoint *d_kps_un, float *d_u_right, float *d_depth_out) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "null handle");
    if (nframes <= 0 || cap <= 0 || !d_kps || !d_counts || !d_u_right || !d_depth_out || !camera4 || ndist < 0 || ndist > 14 ||
        (ndist > 0 && !dist))
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    orbx_status st = rgbd_check(nframes, d_depth, depth_format, width, height, stride, frame_stride);
    if (st != ORBX_OK) return st;
    double K4[4], k14[14]; int identity;
    st = undistort_args(camera4, dist, ndist, K4, k14, &identity);
    if (st != ORBX_OK) return st;
    if (h->host_only) return orbx_fail(ORBX_NO_DEVICE, "no device handle");
    HIPCHK(hipSetDevice(h->dev));
    OrbxRgbdArgs a;
    a.depth = (const uint8_t *)d_depth; a.frame_stride = frame_stride; a.stride = stride; a.format = depth_format;
    a.width = width; a.height = height; a.scale_f32 = rgbd_scale_f32(depth_format, depth_scale); a.scale = depth_scale; a.mbf = mbf;
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_rgbd(h->stream, nframes, cap, cap, K4, k14, identity, a, d_kps, nullptr, d_counts, d_kps_un, d_u_right, d_depth_out); }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    return ORBX_OK;
}

extern "C" orbx_status orbx_rgbd_depth(orbx_handle *h, const orbx_keypoint *kps, const orbx_keypoint *kps_un, int n, const void *depth,
                                       int depth_format, int width, int height, int stride, float depth_scale, float mbf,
                                       float *u_right, float *depth_out) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "null handle");
    if (n < 0 || (n > 0 && (!kps || !kps_un || !u_right || !depth_out))) return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    orbx_status st = rgbd_check(1, depth, depth_format, width, height, stride, 0);
    if (st != ORBX_OK) return st;
    if (h->host_only) return orbx_fail(ORBX_NO_DEVICE, "no device handle");
    if (n == 0) return ORBX_OK;
    HIPCHK(hipSetDevice(h->dev));
    const size_t span = (size_t)depth_span(depth_format, width, height, stride);
    const size_t kb = (size_t)n * sizeof(orbx_keypoint), fb = (size_t)n * sizeof(float);
    st = scratch_reserve(h, 2 * ((kb + 255) & ~(size_t)255) + ((2 * fb + 255) & ~(size_t)255) + ((span + 255) & ~(size_t)255) + 256);
    if (st != ORBX_OK) return st;
    orbx_keypoint *dk = scratch_take<orbx_keypoint>(h, n), *dku = scratch_take<orbx_keypoint>(h, n);
    float *dout = scratch_take<float>(h, 2 * (size_t)n);
    uint8_t *dd = scratch_take<uint8_t>(h, span);
    const double K4[4] = {1, 1, 0, 0}, k14[14] = {0};
    OrbxRgbdArgs a;
    a.depth = dd; a.frame_stride = 0; a.stride = stride; a.format = depth_format; a.width = width; a.height = height;
    a.scale_f32 = rgbd_scale_f32(depth_format, depth_scale); a.scale = depth_scale; a.mbf = mbf;
#define SYNCCHK(expr)                                                                                                       \
    do {                                                                                                                    \
        hipError_t _e = (expr);                                                                                             \
        if (_e != hipSuccess) { hipStreamSynchronize(h->stream); return orbx_fail(ORBX_HIP_ERROR, std::string(#expr) + ": " + hipGetErrorString(_e)); } \
    } while (0)
    SYNCCHK(hipMemcpyAsync(dk, kps, kb, hipMemcpyHostToDevice, h->stream));
    SYNCCHK(hipMemcpyAsync(dku, kps_un, kb, hipMemcpyHostToDevice, h->stream));
    SYNCCHK(hipMemcpyAsync(dd, depth, span, hipMemcpyHostToDevice, h->stream));
    orbx_launch_rgbd(h->stream, 1, n, n, K4, k14, 1, a, dk, dku, nullptr, nullptr, dout, dout + n);
    SYNCCHK(hipGetLastError());
    SYNCCHK(hipMemcpyAsync(u_right, dout, fb, hipMemcpyDeviceToHost, h->stream));
    SYNCCHK(hipMemcpyAsync(depth_out, dout + n, fb, hipMemcpyDeviceToHost, h->stream));
    SYNCCHK(hipStreamSynchronize(h->stream));
#undef SYNCCHK
    return ORBX_OK;
}

extern "C" orbx_status orbx_extract_rgbd_batch(orbx_handle *h, int nframes, const uint8_t *imgs, int width, int height, int stride,
                                               int64_t frame_stride, const void *depth, int depth_format, int depth_stride,
                                               int64_t depth_frame_stride, float depth_scale, const float *camera4, const float *dist,
                                               int ndist, float mbf, orbx_keypoint *kps, orbx_keypoint *kps_un, uint8_t *desc,
                                               int32_t *counts, float *u_right, float *depth_out, int cap) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "null handle");
    if (nframes <= 0 || !imgs || width <= 0 || height <= 0) return orbx_fail(ORBX_EMPTY_IMAGE, "empty image");
    if (!kps || !kps_un || !desc || !counts || !u_right || !depth_out || cap <= 0 || !camera4 || ndist < 0 || ndist > 14 ||
        (ndist > 0 && !dist))
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    orbx_status st = rgbd_check(nframes, depth, depth_format, width, height, depth_stride, depth_frame_stride);
    if (st != ORBX_OK) return st;
    RgbdHost rg;
    st = undistort_args(camera4, dist, ndist, rg.K4, rg.k14, &rg.identity);
    if (st != ORBX_OK) return st;
    if (h->host_only) return orbx_fail(ORBX_NO_DEVICE, "no device handle");
    rg.depth = (const uint8_t *)depth; rg.format = depth_format; rg.stride = depth_stride;
    rg.frame_stride = nframes > 1 ? depth_frame_stride : depth_span(depth_format, width, height, depth_stride);
    rg.scale = depth_scale; rg.mbf = mbf; rg.scale_f32 = rgbd_scale_f32(depth_format, depth_scale);
    rg.kps_un = kps_un; rg.u_right = u_right; rg.depth_out = depth_out;
    return extract_host(h, nframes, imgs, width, height, stride, frame_stride, kps, desc, counts, cap, &rg);
}

extern "C" orbx_status orbx_extract(orbx_handle *h, const uint8_t *img, int width, int height, int stride,
                                    orbx_keypoint *kps, uint8_t *desc, int cap, int *n) {
    if (!n) return orbx_fail(ORBX_BAD_ARGUMENT, "null count pointer");
    int32_t cnt = 0;
    orbx_status st = orbx_extract_batch(h, 1, img, width, height, stride, (int64_t)stride * height, kps, desc, &cnt, cap);
    if (st == ORBX_OK || st == ORBX_CAPACITY) *n = cnt;
    return st;
}

// ---------------------------------------------------------------- (f)2: Frame::UndistortKeyPoints / ComputeImageBounds
// (src/Frame.cc:770-865): cv::undistortPoints(K, D, R = I, P = K) on the device (k_undistort).  camera4 = fx, fy, cx, cy
// (mK), dist = mDistCoef (k1, k2, p1, p2[, k3 ...], up to 14).  dist[0] == 0 copies the keypoints (:772-776).
extern "C" orbx_status orbx_undistort_keypoints_device(orbx_handle *h, int nframes, const orbx_keypoint *d_kps,
                                                       const int32_t *d_counts, int cap, const float *camera4, const float *dist,
                                                       int ndist, orbx_keypoint *d_kps_un) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no device handle");
    if (nframes <= 0 || cap <= 0 || !d_kps || !d_counts || !d_kps_un || !camera4 || ndist < 0 || ndist > 14 || (ndist > 0 && !dist))
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    double K4[4], k14[14]; int identity;
    orbx_status st = undistort_args(camera4, dist, ndist, K4, k14, &identity);
    if (st != ORBX_OK) return st;
    if (h->host_only) return orbx_fail(ORBX_NO_DEVICE, "no device handle");
    HIPCHK(hipSetDevice(h->dev));
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_undistort(h->stream, nframes, cap, cap, K4, k14, identity, d_kps, d_counts, d_kps_un); }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    return ORBX_OK;
}
extern "C" orbx_status orbx_undistort_keypoints(orbx_handle *h, const orbx_keypoint *kps, int n, const float *camera4,
                                                const float *dist, int ndist, orbx_keypoint *kps_un) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no device handle");
    if (n < 0 || (n > 0 && (!kps || !kps_un)) || !camera4 || ndist < 0 || ndist > 14 || (ndist > 0 && !dist))
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    double K4[4], k14[14]; int identity;
    orbx_status st = undistort_args(camera4, dist, ndist, K4, k14, &identity);
    if (st != ORBX_OK) return st;
    if (h->host_only) return orbx_fail(ORBX_NO_DEVICE, "no device handle");
    if (n == 0) return ORBX_OK;
    HIPCHK(hipSetDevice(h->dev));
    st = scratch_reserve(h, 2 * pad256((size_t)n * sizeof(orbx_keypoint)));
    if (st != ORBX_OK) return st;
    orbx_keypoint *din = scratch_take<orbx_keypoint>(h, n), *dout = scratch_take<orbx_keypoint>(h, n);
    HIPCHK(hipMemcpyAsync(din, kps, (size_t)n * sizeof(orbx_keypoint), hipMemcpyHostToDevice, h->stream));
    orbx_launch_undistort(h->stream, 1, n, n, K4, k14, identity, din, nullptr, dout);
    HIPCHK(hipMemcpyAsync(kps_un, dout, (size_t)n * sizeof(orbx_keypoint), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ORBX_OK;
}
// Frame::ComputeImageBounds (:830-865): the four image corners through the same kernel
extern "C" orbx_status orbx_image_bounds(orbx_handle *h, int cols, int rows, const float *camera4, const float *dist, int ndist,
                                         float *bounds4) {
    if (!bounds4 || cols <= 0 || rows <= 0) return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    if (dist) {   // the tilt rule holds for the identity answer too: one rule for every entry point
        double K4[4], k14[14]; int identity;
        const orbx_status st = undistort_args(nullptr, dist, ndist, K4, k14, &identity);
        if (st != ORBX_OK) return st;
    }
    if (ndist < 1 || !dist || dist[0] == 0.0f) {
        bounds4[0] = 0.0f; bounds4[1] = (float)cols; bounds4[2] = 0.0f; bounds4[3] = (float)rows;
        return ORBX_OK;
    }
    orbx_keypoint c[4], u[4];
    memset(c, 0, sizeof(c));
    c[1].x = (float)cols; c[2].y = (float)rows; c[3].x = (float)cols; c[3].y = (float)rows;
    const orbx_status st = orbx_undistort_keypoints(h, c, 4, camera4, dist, ndist, u);
    if (st != ORBX_OK) return st;
    bounds4[0] = std::min(u[0].x, u[2].x); bounds4[1] = std::max(u[1].x, u[3].x);
    bounds4[2] = std::min(u[0].y, u[1].y); bounds4[3] = std::max(u[2].y, u[3].y);
    return ORBX_OK;
}
