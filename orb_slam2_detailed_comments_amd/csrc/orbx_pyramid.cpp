// orbx_pyramid.cpp -- everything that reads the last batch's slab, behind the C ABI: pyramid level access (with the late
// level 0 of an in-place batch), the per-stage inspection calls, and Frame::ComputeStereoMatches over both eyes' pyramids.
#include <cstring>
#include <algorithm>
#include <utility>
#include <vector>
#include "orbx_handle.h"

// ---------------------------------------------------------------- pyramid access
// byte offset of mvImagePyramid[level] inside one frame's slab: the padded level, or the view at (org, org) of it
static inline size_t level_view_off(const OrbxLevelGeom &L) { return (size_t)L.off + (size_t)L.org * L.pitch + L.org; }
static orbx_status check_level(orbx_handle *h, int frame, int level) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "null handle");
    if (!h->configured || h->last_batch == 0) return orbx_fail(ORBX_BAD_ARGUMENT, "no frame extracted yet");
    if (level < 0 || level >= h->p.nlevels || frame < 0 || frame >= h->last_batch) return orbx_fail(ORBX_BAD_ARGUMENT, "frame/level out of range");
    return ORBX_OK;
}
extern "C" orbx_status orbx_pyramid_level_info(orbx_handle *h, int level, int *width, int *height, int *pitch) {
    orbx_status st = check_level(h, 0, level);
    if (st != ORBX_OK) return st;
    if (width) *width = h->geom.lv[level].vw;    // mvImagePyramid[level]: the padded level (fork) or the view inside it (upstream)
    if (height) *height = h->geom.lv[level].vh;
    if (pitch) *pitch = h->geom.lv[level].pitch;
    return ORBX_OK;
}
// The slab's padded level 0 of the last batch, written late: an in-place batch (run_chunk) left it out.  Runs k_pyr_l0 on the
// handle's stream from the recorded input, at most once per batch; its status / cursor resets go to scratch words.
static orbx_status ensure_level0(orbx_handle *h) {
    if (!h->l0_pending) return ORBX_OK;
    HIPCHK(hipSetDevice(h->dev));
    { ProfScope ps(h, ORBX_K_PYR_L0);
      orbx_launch_pyr_l0(h->stream, h->dg, h->last_batch, h->l0_src.img, h->l0_src.W, h->l0_src.H, h->l0_src.stride,
                         h->l0_src.frame_stride, h->d_pyr, h->d_l0_scratch, h->d_l0_scratch + h->p.max_batch); }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, std::string("late level 0: ") + hipGetErrorString(e));
    h->l0_pending = false;
    return ORBX_OK;
}
extern "C" orbx_status orbx_pyramid_level_device(orbx_handle *h, int frame, int level, const uint8_t **d_ptr) {
    orbx_status st = check_level(h, frame, level);
    if (st != ORBX_OK) return st;
    if (level == 0) {   // the other levels were written by the batch itself
        st = ensure_level0(h);
        if (st != ORBX_OK) return st;
    }
    *d_ptr = h->d_pyr + (size_t)frame * h->geom.pyr_bytes + level_view_off(h->geom.lv[level]);
    return ORBX_OK;
}
static orbx_status copy_level(orbx_handle *h, const uint8_t *slab, int frame, int level, uint8_t *dst, int dst_stride) {
    orbx_status st = check_level(h, frame, level);
    if (st != ORBX_OK) return st;
    const OrbxLevelGeom &L = h->geom.lv[level];
    if (!dst || dst_stride < L.vw) return orbx_fail(ORBX_BAD_ARGUMENT, "dst / dst_stride");
    HIPCHK(hipSetDevice(h->dev));
    if (level == 0 && slab == h->d_pyr) {   // (the blurred slab's level 0 was built behind its own ensure_level0)
        st = ensure_level0(h);
        if (st != ORBX_OK) return st;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy2D(dst, dst_stride, slab + (size_t)frame * h->geom.pyr_bytes + level_view_off(L), L.pitch, L.vw, L.vh,
                       hipMemcpyDeviceToHost));
    return ORBX_OK;
}
extern "C" orbx_status orbx_pyramid_level_copy(orbx_handle *h, int frame, int level, uint8_t *dst, int dst_stride) {
    return copy_level(h, h ? h->d_pyr : nullptr, frame, level, dst, dst_stride);
}
extern "C" orbx_status orbx_debug_blur_copy(orbx_handle *h, int frame, int level, uint8_t *dst, int dst_stride) {
    orbx_status st = check_level(h, frame, level);
    if (st != ORBX_OK) return st;
    if (!h->blur_valid) {  // stand-alone k_blur over the resident pyramid (same arithmetic as the fused path)
        HIPCHK(hipSetDevice(h->dev));
        st = ensure_level0(h);
        if (st != ORBX_OK) return st;
        if (!h->d_blur) {      // the blurred slab only exists for inspection: allocated on first request
            HIPCHK(hipMalloc(&h->d_blur, (size_t)h->p.max_batch * h->geom.pyr_bytes + 256));
            HIPCHK(hipMemsetAsync(h->d_blur, 0, (size_t)h->p.max_batch * h->geom.pyr_bytes, h->stream));   // ordered with k_blur below
        }
        { ProfScope ps(h, ORBX_K_BLUR);
          orbx_launch_blur(h->stream, h->dg, h->last_batch, h->d_pyr, h->d_blur); }
        h->blur_valid = true;
    }
    return copy_level(h, h->d_blur, frame, level, dst, dst_stride);
}

// ---------------------------------------------------------------- per-stage inspection
extern "C" orbx_status orbx_debug_candidates(orbx_handle *h, int frame, int level, orbx_keypoint *out, int cap, int *n) {
    orbx_status st = check_level(h, frame, level);
    if (st != ORBX_OK) return st;
    HIPCHK(hipSetDevice(h->dev));
    HIPCHK(hipStreamSynchronize(h->stream));
    const OrbxLevelGeom &L = h->geom.lv[level];
    int cnt = 0;
    HIPCHK(hipMemcpy(&cnt, h->d_cand_count + frame * h->p.nlevels + level, sizeof(int), hipMemcpyDeviceToHost));
    if (n) *n = cnt;
    const int m = std::min(cnt, L.cand_cap);
    std::vector<uint2> rec(std::max(m, 1));
    if (m > 0)
        HIPCHK(hipMemcpy(rec.data(), h->d_dense + (size_t)frame * h->geom.cand_total + L.cand_begin, (size_t)m * sizeof(uint2),
                         hipMemcpyDeviceToHost));
    for (int i = 0; i < m && i < cap; ++i) {
        orbx_keypoint k;
        k.x = (float)(rec[i].x & 0xfff); k.y = (float)((rec[i].x >> 12) & 0xfff);
        k.size = 7.f; k.angle = -1.f; k.response = (float)(rec[i].x >> 24);
        k.octave = 0; k.class_id = (int32_t)(rec[i].y & 0xffffff);  // emission-order key (debug only)
        out[i] = k;
    }
    if (cnt > L.cand_cap || m > cap) return orbx_fail(ORBX_CAPACITY, "candidate capacity");
    return ORBX_OK;
}

extern "C" orbx_status orbx_debug_level_keypoints(orbx_handle *h, int frame, int level, orbx_keypoint *out, int cap, int *n) {
    orbx_status st = check_level(h, frame, level);
    if (st != ORBX_OK) return st;
    HIPCHK(hipSetDevice(h->dev));
    HIPCHK(hipStreamSynchronize(h->stream));
    const OrbxLevelGeom &L = h->geom.lv[level];
    int cnt = 0;
    HIPCHK(hipMemcpy(&cnt, h->d_lvl_count + frame * h->p.nlevels + level, sizeof(int), hipMemcpyDeviceToHost));
    if (n) *n = cnt;
    std::vector<uint32_t> pos(std::max(cnt, 1));
    std::vector<float> ang(std::max(cnt, 1));
    if (cnt > 0) {
        HIPCHK(hipMemcpy(pos.data(), h->d_lvl_kp + (size_t)frame * h->geom.kp_total + L.kp_begin, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ang.data(), h->d_lvl_angle + (size_t)frame * h->geom.kp_total + L.kp_begin, cnt * sizeof(float), hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < cnt && i < cap; ++i) {
        orbx_keypoint k;
        k.x = (float)((pos[i] & 0xfff) + ORBX_EDGE - 3); k.y = (float)(((pos[i] >> 12) & 0xfff) + ORBX_EDGE - 3);
        k.size = L.size; k.angle = ang[i]; k.response = (float)(pos[i] >> 24); k.octave = level; k.class_id = -1;
        out[i] = k;
    }
    if (cnt > cap) return orbx_fail(ORBX_CAPACITY, "output capacity");
    return ORBX_OK;
}

extern "C" orbx_status orbx_debug_fast_groups(orbx_handle *h, int *level0, int *total) {
    if (!h || !h->configured) return orbx_fail(ORBX_BAD_ARGUMENT, "no batch has been extracted on this handle");
    if (level0) *level0 = h->l0_groups;
    if (total) *total = (int)h->geom.fast_groups.size();
    return ORBX_OK;
}
// the launchers' size rules (orbx_launch.h), pure arithmetic: host-only handles answer too
extern "C" orbx_status orbx_debug_match_plan(orbx_handle *h, int npairs, int out_stride, int *qt, int *nsplit) {
    if (!h || npairs <= 0 || out_stride <= 0) return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    const OrbxMatchPlan plan = orbx_match_plan(npairs, out_stride, h->match_kernel);
    if (qt) *qt = plan.qt;
    if (nsplit) *nsplit = plan.nsplit;
    return ORBX_OK;
}
extern "C" orbx_status orbx_debug_fast_gpw(orbx_handle *h, int nframes, int ngroups, int *gpw) {
    if (!h || nframes <= 0 || ngroups <= 0) return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    if (!h->configured) {   // what configure() would store
        const orbx_status st = read_fast_gpw(h);
        if (st != ORBX_OK) return st;
    }
    if (gpw) *gpw = orbx_fast_gpw(nframes, ngroups, h->fast_gpw);
    return ORBX_OK;
}
extern "C" orbx_status orbx_debug_describe_pattern(int8_t *lane_i8_1024, float *lane_f32_1024) {
    if (!lane_i8_1024 || !lane_f32_1024) return orbx_fail(ORBX_BAD_ARGUMENT, "null table");
    orbx_pattern_lane_tables((signed char *)lane_i8_1024, lane_f32_1024);
    return ORBX_OK;
}

// ---------------------------------------------------------------- a16: ComputeStereoMatches (src/Frame.cc:880-1176)
// mvImagePyramid of both eyes as the match reads it: the padded levels (fork) or the views inside them (upstream)
static OrbxStereoGeom stereo_geom(const orbx_handle *hl, float mb, float mbf) {
    OrbxStereoGeom sg;
    memset(&sg, 0, sizeof(sg));
    sg.nlevels = hl->p.nlevels; sg.nrows0 = hl->geom.lv[0].vh; sg.mb = mb; sg.mbf = mbf;
    for (int l = 0; l < sg.nlevels; ++l) {
        const OrbxLevelGeom &L = hl->geom.lv[l];
        sg.scale[l] = hl->tab.scale[l]; sg.inv_scale[l] = hl->tab.inv_scale[l];
        sg.pw[l] = L.vw; sg.ph[l] = L.vh; sg.pitch[l] = L.pitch;
        sg.off[l] = (long long)level_view_off(L);
    }
    return sg;
}
extern "C" orbx_status orbx_stereo_match(orbx_handle *hl, orbx_handle *hr, int frame_left, int frame_right,
                                         const orbx_keypoint *kl, const uint8_t *dl, int nl, const orbx_keypoint *kr,
                                         const uint8_t *dr, int nr, float mb, float mbf, float *u_right, float *depth,
                                         int *nmatches_out) {
    if (!hl || !hr || hl->host_only || hr->host_only) return orbx_fail(ORBX_BAD_ARGUMENT, "two device handles are required");
    if (nl < 0 || nr < 0 || nr > 65535 || (nl > 0 && (!kl || !dl || !u_right || !depth)) || (nr > 0 && (!kr || !dr)) ||
        !(mb > 0.f))
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    orbx_status st = check_level(hl, frame_left, 0);
    if (st != ORBX_OK) return st;
    st = check_level(hr, frame_right, 0);
    if (st != ORBX_OK) return st;
    if (hl->dev != hr->dev || hl->geom.width != hr->geom.width || hl->geom.height != hr->geom.height ||
        hl->p.nlevels != hr->p.nlevels || hl->p.scale_factor != hr->p.scale_factor || hl->p.pyramid_mode != hr->p.pyramid_mode)
        return orbx_fail(ORBX_BAD_ARGUMENT, "left and right extractor must share device, image size, pyramid parameters and pyramid_mode");
    if (nmatches_out) *nmatches_out = 0;
    if (nl == 0) return ORBX_OK;
    HIPCHK(hipSetDevice(hl->dev));
    for (orbx_handle *hh : {hl, hr}) {          // the match reads both padded level-0 images (then written eagerly: see run_chunk)
        if (hh->l0_pending) hh->l0_eager_sticky = true;
        st = ensure_level0(hh);
        if (st != ORBX_OK) return st;
    }
    HIPCHK(hipStreamSynchronize(hr->stream));   // the right pyramid is read from the left handle's stream
    const OrbxStereoGeom sg = stereo_geom(hl, mb, mbf);
    st = scratch_reserve(hl, pad256((size_t)nl * sizeof(orbx_keypoint)) + pad256((size_t)nl * 32) +
                                 pad256((size_t)std::max(nr, 1) * sizeof(orbx_keypoint)) + pad256((size_t)std::max(nr, 1) * 32) +
                                 3 * pad256((size_t)nl * sizeof(float)) + pad256((size_t)(sg.nrows0 + 1) * sizeof(int)) +
                                 pad256((size_t)orbx_stereo_items_per_pair(sg, std::max(nr, 1)) * sizeof(uint2)));
    if (st != ORBX_OK) return st;
    orbx_keypoint *dkl = scratch_take<orbx_keypoint>(hl, nl);
    uint8_t *ddl = scratch_take<uint8_t>(hl, (size_t)nl * 32);
    orbx_keypoint *dkr = scratch_take<orbx_keypoint>(hl, std::max(nr, 1));
    uint8_t *ddr = scratch_take<uint8_t>(hl, (size_t)std::max(nr, 1) * 32);
    float *du = scratch_take<float>(hl, nl), *dz = scratch_take<float>(hl, nl);
    int *dsad = scratch_take<int>(hl, nl);
    int *drow = scratch_take<int>(hl, (size_t)sg.nrows0 + 1);
    uint2 *ditems = scratch_take<uint2>(hl, (size_t)orbx_stereo_items_per_pair(sg, std::max(nr, 1)));
    HIPCHK(hipMemcpyAsync(dkl, kl, (size_t)nl * sizeof(orbx_keypoint), hipMemcpyHostToDevice, hl->stream));
    HIPCHK(hipMemcpyAsync(ddl, dl, (size_t)nl * 32, hipMemcpyHostToDevice, hl->stream));
    if (nr > 0) {
        HIPCHK(hipMemcpyAsync(dkr, kr, (size_t)nr * sizeof(orbx_keypoint), hipMemcpyHostToDevice, hl->stream));
        HIPCHK(hipMemcpyAsync(ddr, dr, (size_t)nr * 32, hipMemcpyHostToDevice, hl->stream));
    }
    { ProfScope ps(hl, ORBX_K_MATCH);
      orbx_launch_stereo(hl->stream, sg, dkl, ddl, nl, dkr, ddr, nr, hl->d_pyr + (size_t)frame_left * hl->geom.pyr_bytes,
                         hr->d_pyr + (size_t)frame_right * hr->geom.pyr_bytes, du, dz, dsad, drow, ditems); }
    std::vector<int> sad(nl);
    HIPCHK(hipMemcpyAsync(u_right, du, (size_t)nl * sizeof(float), hipMemcpyDeviceToHost, hl->stream));
    HIPCHK(hipMemcpyAsync(depth, dz, (size_t)nl * sizeof(float), hipMemcpyDeviceToHost, hl->stream));
    HIPCHK(hipMemcpyAsync(sad.data(), dsad, (size_t)nl * sizeof(int), hipMemcpyDeviceToHost, hl->stream));
    hipError_t e = hipStreamSynchronize(hl->stream);
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    // median cut (:1160-1175): sort (SAD, index), drop everything at or above 1.5 * 1.4 * median
    std::vector<std::pair<int, int>> v;
    for (int i = 0; i < nl; ++i) if (sad[i] >= 0) v.push_back({sad[i], i});
    int kept = (int)v.size();
    if (!v.empty()) {
        std::sort(v.begin(), v.end());
        const float median = (float)v[v.size() / 2].first;
        const float thDist = 1.5f * 1.4f * median;
        for (int i = (int)v.size() - 1; i >= 0; --i) {
            if ((float)v[i].first < thDist) break;
            u_right[v[i].second] = -1; depth[v[i].second] = -1; --kept;
        }
    }
    if (nmatches_out) *nmatches_out = kept;
    return ORBX_OK;
}

// Batched, device-resident Frame::ComputeStereoMatches: pair p = frame p of the last extraction of `hl` (left) and of
// `hr` (right); keypoints / descriptors / counts are the device buffers orbx_extract_batch_device filled (stride `cap`
// records per frame).  The median cut (:1160-1175) also runs on the device (k_stereo_cut), nothing returns to the host.
extern "C" orbx_status orbx_stereo_match_batch_device(orbx_handle *hl, orbx_handle *hr, int npairs, const orbx_keypoint *d_kl,
                                                      const uint8_t *d_dl, const int32_t *d_nl, const orbx_keypoint *d_kr,
                                                      const uint8_t *d_dr, const int32_t *d_nr, int cap, float mb, float mbf,
                                                      float *d_u_right, float *d_depth, int32_t *d_nmatches) {
    if (!hl || !hr || hl->host_only || hr->host_only) return orbx_fail(ORBX_BAD_ARGUMENT, "two device handles are required");
    if (npairs <= 0 || cap <= 0 || cap > 65535 || !d_kl || !d_dl || !d_nl || !d_kr || !d_dr || !d_nr || !d_u_right || !d_depth ||
        !d_nmatches || !(mb > 0.f))
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    // hl == hr: both eyes went through ONE batch of 2 * npairs images (left images first): the right pyramids are frames
    // npairs .. 2 npairs - 1 of that handle (half as many launches per stereo frame as two handles need)
    const bool one_batch = hl == hr;
    orbx_status st = check_level(hl, (one_batch ? 2 * npairs : npairs) - 1, 0);
    if (st != ORBX_OK) return st;
    st = check_level(hr, npairs - 1, 0);
    if (st != ORBX_OK) return st;
    if (hl->dev != hr->dev || hl->geom.width != hr->geom.width || hl->geom.height != hr->geom.height ||
        hl->p.nlevels != hr->p.nlevels || hl->p.scale_factor != hr->p.scale_factor || hl->p.pyramid_mode != hr->p.pyramid_mode)
        return orbx_fail(ORBX_BAD_ARGUMENT, "left and right extractor must share device, image size, pyramid parameters and pyramid_mode");
    HIPCHK(hipSetDevice(hl->dev));
    // The match reads the padded level 0 of both eyes: an in-place batch writes it now, on its own handle's stream, and the
    // handle goes back to the eager k_pyr_l0 for its later batches (a stereo pipeline would pay the late copy every time)
    for (orbx_handle *hh : {hl, hr}) {
        if (hh->l0_pending) hh->l0_eager_sticky = true;
        st = ensure_level0(hh);
        if (st != ORBX_OK) return st;
    }
    // The reference extracts the two eyes on two threads (src/Frame.cc:158-168); here that is two handles on two streams.  The
    // match runs on the left stream: it waits for the right stream's work so far (an event, no host synchronisation) ...
    const bool two_streams = hr->stream != hl->stream;
    if (two_streams) {
        HIPCHK(hipEventRecord(hr->ev_stereo, hr->stream));
        HIPCHK(hipStreamWaitEvent(hl->stream, hr->ev_stereo, 0));
    }
    const OrbxStereoGeom sg = stereo_geom(hl, mb, mbf);
    const size_t ipp = (size_t)orbx_stereo_items_per_pair(sg, cap);
    st = scratch_reserve(hl, pad256((size_t)npairs * cap * sizeof(int)) + pad256((size_t)npairs * (sg.nrows0 + 1) * sizeof(int)) +
                                 pad256((size_t)npairs * ipp * sizeof(uint2)));
    if (st != ORBX_OK) return st;
    int *dsad = scratch_take<int>(hl, (size_t)npairs * cap);
    int *drow = scratch_take<int>(hl, (size_t)npairs * (sg.nrows0 + 1));
    uint2 *ditems = scratch_take<uint2>(hl, (size_t)npairs * ipp);
    { ProfScope ps(hl, ORBX_K_MATCH);
      orbx_launch_stereo_batch(hl->stream, sg, npairs, cap, d_kl, d_dl, d_nl, d_kr, d_dr, d_nr, hl->d_pyr,
                               hr->d_pyr + (one_batch ? (size_t)npairs * (size_t)hl->geom.pyr_bytes : 0),
                               (long long)hl->geom.pyr_bytes, d_u_right, d_depth, dsad, d_nmatches, drow, ditems); }
    if (two_streams) {   // ... and whatever the right stream does next (the next pair's pyramids) waits for the match that reads this one's
        HIPCHK(hipEventRecord(hl->ev_stereo, hl->stream));
        HIPCHK(hipStreamWaitEvent(hr->stream, hl->ev_stereo, 0));
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    return ORBX_OK;
}
