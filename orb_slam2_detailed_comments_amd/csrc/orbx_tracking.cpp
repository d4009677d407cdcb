// orbx_tracking.cpp -- the tracking matchers behind the C ABI: the two SearchByProjection policies, per call on the host over
// gated candidate lists and batched on the device (orbx_track.h), MapPoint::PredictScale, and Tracking::SearchLocalPoints.
#include <cmath>
#include <cstring>
#include <vector>
#include "orbx_handle.h"
#include "orbx_gate.h"

// ---------------------------------------------------------------- a14: SearchByProjection(Frame&, const Frame&, th, bMono)
// (src/ORBmatcher.cc:1702-1871; caller TrackWithMotionModel src/Tracking.cc:1430,1445).  Host: projection (fp32, same
// operation order as the reference incl. the contraction selected by fp_mode).  GPU: grid of the current frame, the
// windows' candidates and their Hamming distances to the MapPoints' representative descriptors (orbx_gate_lists).
// Host: the occupancy rule and the rotation histogram over those lists -- order-dependent.
static inline float orbx_gemm3(const float *a, const float *b, float c) {  // cv::gemm 3x3 * 3x1 float special case
    const float t = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    return (float)((double)t * 1.0 + (double)c * 1.0);
}

extern "C" orbx_status orbx_search_by_projection_frame(orbx_handle *h, const orbx_frame_view *cur,
                                                       const orbx_last_frame_view *last, float th, int mono,
                                                       int check_orientation, int32_t *matched_last, int *nmatches_out) {
    if (!h || h->host_only) return orbx_fail(h ? ORBX_NO_DEVICE : ORBX_BAD_ARGUMENT, "no device handle");
    if (!cur || !last || !matched_last || !nmatches_out || cur->n < 0 || last->n < 0)
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    const int nc = cur->n, nl = last->n, HISTO = 30, TH_HIGH_ = 100;
    *nmatches_out = 0;
    for (int i = 0; i < nc; ++i) matched_last[i] = -1;
    if (nc == 0 || nl == 0) return ORBX_OK;
    if (!cur->keys_un || !cur->desc || !cur->u_right || !last->keys_un || !last->has_map_point || !last->world_pos ||
        !last->mp_desc || !last->observations)
        return orbx_fail(ORBX_BAD_ARGUMENT, "null frame field");
    const bool fma_mode = h->p.fp_mode == ORBX_FP_GCC_FMA;
    float Rcw[9], tcw[3], Rlw[9], tlw[3], twc[3], tlc[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { Rcw[3 * r + c] = cur->Tcw[4 * r + c]; Rlw[3 * r + c] = last->Tcw[4 * r + c]; }
        tcw[r] = cur->Tcw[4 * r + 3]; tlw[r] = last->Tcw[4 * r + 3];
    }
    for (int r = 0; r < 3; ++r) {
        const float t = Rcw[0 + r] * tcw[0] + Rcw[3 + r] * tcw[1] + Rcw[6 + r] * tcw[2];
        twc[r] = (float)((double)t * -1.0);
    }
    for (int r = 0; r < 3; ++r) tlc[r] = orbx_gemm3(&Rlw[3 * r], twc, tlw[r]);
    const bool bForward = tlc[2] > cur->mb && !mono, bBackward = -tlc[2] > cur->mb && !mono;
    // pass 1 (host, independent of the selection state): project every MapPoint of the last frame, derive its window and
    // octave band (:1742-1783).  pass 2 (GPU): the windows' candidates + Hamming distances.  pass 3 (host): the selection.
    std::vector<DGateQuery> gq((size_t)nl);
    std::vector<float> q_invz((size_t)nl, 0.f), q_u((size_t)nl, 0.f);
    for (int i = 0; i < nl; ++i) {
        gq[i].r = -1.0f; gq[i].x = gq[i].y = 0.f; gq[i].min_level = gq[i].max_level = -1;
        if (!last->has_map_point[i]) continue;
        float pc[3];
        for (int r = 0; r < 3; ++r) pc[r] = orbx_gemm3(&Rcw[3 * r], last->world_pos + 3 * (size_t)i, tcw[r]);
        const float invzc = (float)(1.0 / pc[2]);
        if (invzc < 0) continue;
        float u, v;
        if (fma_mode) { u = std::fmaf(cur->fx * pc[0], invzc, cur->cx); v = std::fmaf(cur->fy * pc[1], invzc, cur->cy); }
        else { u = cur->fx * pc[0] * invzc + cur->cx; v = cur->fy * pc[1] * invzc + cur->cy; }
        if (u < cur->min_x || u > cur->max_x || v < cur->min_y || v > cur->max_y) continue;
        const int oct = last->keys_un[i].octave;
        if (oct < 0 || oct >= h->p.nlevels) continue;
        gq[i].x = u; gq[i].y = v; gq[i].r = th * h->tab.scale[oct];
        if (bForward) { gq[i].min_level = oct; gq[i].max_level = -1; }
        else if (bBackward) { gq[i].min_level = 0; gq[i].max_level = oct; }
        else { gq[i].min_level = oct - 1; gq[i].max_level = oct + 1; }
        q_invz[i] = invzc; q_u[i] = u;
    }
    OrbxGateLists gl;
    { const orbx_status st = orbx_gate_lists(h, cur->keys_un, cur->desc, nc, cur->min_x, cur->max_x, cur->min_y, cur->max_y,
                                             gq.data(), last->mp_desc, nl, gl);
      if (st != ORBX_OK) return st; }
    std::vector<std::vector<int>> rotHist(HISTO);
    const float factor = HISTO / 360.0f;  // fork value (src/ORBmatcher.cc:1713)
    int nmatches = 0;
    for (int i = 0; i < nl; ++i) {
        if (gq[i].r < 0.f) continue;
        const float invzc = q_invz[i], u = q_u[i], radius = gq[i].r;
        const int ncand = gl.count(i);
        if (ncand == 0) continue;
        const uint32_t *cl = gl.list(i);
        int bestDist = 256, bestIdx2 = -1;
        for (int c = 0; c < ncand; ++c) {
            const int i2 = OrbxGateLists::idx(cl[c]);
            if (matched_last[i2] >= 0 && last->observations[matched_last[i2]] > 0) continue;
            if (cur->u_right[i2] > 0) {
                const float ur = fma_mode ? std::fmaf(-cur->mbf, invzc, u) : u - cur->mbf * invzc;
                if (fabsf(ur - cur->u_right[i2]) > radius) continue;
            }
            const int dist = OrbxGateLists::dist(cl[c]);
            if (dist < bestDist) { bestDist = dist; bestIdx2 = i2; }
        }
        if (bestDist <= TH_HIGH_) {
            matched_last[bestIdx2] = i;
            nmatches++;
            if (check_orientation) {
                float rot = last->keys_un[i].angle - cur->keys_un[bestIdx2].angle;
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)roundf(rot * factor);
                if (bin == HISTO) bin = 0;
                if (bin >= 0 && bin < HISTO) rotHist[bin].push_back(bestIdx2);
            }
        }
    }
    if (check_orientation) {
        int32_t sizes[30]; int i1, i2, i3;
        for (int i = 0; i < HISTO; ++i) sizes[i] = (int)rotHist[i].size();
        orbx_three_maxima(sizes, HISTO, &i1, &i2, &i3);
        for (int i = 0; i < HISTO; ++i)
            if (i != i1 && i != i2 && i != i3)
                for (int idx2 : rotHist[i]) { matched_last[idx2] = -1; nmatches--; }
    }
    *nmatches_out = nmatches;
    return ORBX_OK;
}

// ---------------------------------------------------------------- (f)1: SearchByProjection(Frame&, vector<MapPoint*>&, th)
// (src/ORBmatcher.cc:69-184, RadiusByViewingCos :187-194; caller Tracking::SearchLocalPoints src/Tracking.cc:1953) --
// the largest per-frame matcher load in steady state.  GPU: the frame's grid, every in-view MapPoint's window candidates
// and their Hamming distances (orbx_gate_lists).  Host: occupancy rule, level-aware ratio test (order-dependent).
extern "C" orbx_status orbx_search_by_projection_mappoints(orbx_handle *h, const orbx_frame_view *frame,
                                                           const int32_t *frame_observations,
                                                           const orbx_mappoint_view *mps, float th, float nnratio,
                                                           int32_t *assigned, int *nmatches_out) {
    if (!h || h->host_only) return orbx_fail(h ? ORBX_NO_DEVICE : ORBX_BAD_ARGUMENT, "no device handle");
    if (!frame || !mps || !assigned || !nmatches_out || frame->n < 0 || mps->n < 0) return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    const int nf = frame->n, nmp = mps->n, TH_HIGH_ = 100;
    *nmatches_out = 0;
    for (int i = 0; i < nf; ++i) assigned[i] = -1;
    if (nf == 0 || nmp == 0) return ORBX_OK;
    if (!frame->keys_un || !frame->desc || !frame->u_right || !frame_observations || !mps->in_view || !mps->proj ||
        !mps->level || !mps->view_cos || !mps->desc || !mps->observations)
        return orbx_fail(ORBX_BAD_ARGUMENT, "null field");
    std::vector<DGateQuery> gq((size_t)nmp);
    bool any = false;
    const bool bFactor = th != 1.0;
    for (int iMP = 0; iMP < nmp; ++iMP) {
        gq[iMP].x = mps->proj[3 * iMP]; gq[iMP].y = mps->proj[3 * iMP + 1]; gq[iMP].r = -1.0f;
        gq[iMP].min_level = gq[iMP].max_level = -1;
        if (!mps->in_view[iMP]) continue;
        const int lvl = mps->level[iMP];
        if (lvl < 0 || lvl >= h->p.nlevels) continue;
        float r = mps->view_cos[iMP] > 0.998 ? 2.5f : 4.0f;
        if (bFactor) r *= th;
        gq[iMP].r = r * h->tab.scale[lvl];
        gq[iMP].min_level = lvl - 1; gq[iMP].max_level = lvl;
        any = true;
    }
    if (!any) return ORBX_OK;
    OrbxGateLists gl;
    { const orbx_status st = orbx_gate_lists(h, frame->keys_un, frame->desc, nf, frame->min_x, frame->max_x, frame->min_y,
                                             frame->max_y, gq.data(), mps->desc, nmp, gl);
      if (st != ORBX_OK) return st; }
    std::vector<int> occ(frame_observations, frame_observations + nf);
    int nmatches = 0;
    for (int iMP = 0; iMP < nmp; ++iMP) {
        if (gq[iMP].r < 0.f) continue;
        const float radius = gq[iMP].r;
        const int nc = gl.count(iMP);
        if (nc == 0) continue;
        const uint32_t *cl = gl.list(iMP);
        int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
        for (int c = 0; c < nc; ++c) {
            const int idx = OrbxGateLists::idx(cl[c]);
            if (occ[idx] > 0) continue;
            if (frame->u_right[idx] > 0 && fabsf(mps->proj[3 * iMP + 2] - frame->u_right[idx]) > radius) continue;
            const int dist = OrbxGateLists::dist(cl[c]);
            if (dist < bestDist) {
                bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = frame->keys_un[idx].octave; bestIdx = idx;
            } else if (dist < bestDist2) {
                bestLevel2 = frame->keys_un[idx].octave; bestDist2 = dist;
            }
        }
        if (bestDist <= TH_HIGH_) {
            if (bestLevel == bestLevel2 && (float)bestDist > nnratio * (float)bestDist2) continue;
            assigned[bestIdx] = iMP;
            occ[bestIdx] = mps->observations[iMP];
            nmatches++;
        }
    }
    *nmatches_out = nmatches;
    return ORBX_OK;
}

// ---------------------------------------------------------------- a14 / (f)1 batched and device-resident (orbx_track.h)
// One call: validation and layout (orbx_track_pack.cpp), all problems' host arrays packed into the page-locked block, ONE upload,
// k_track_project (frame policy) + k_track_cand + k_track_select on the handle's stream.  Nothing is downloaded and nothing is
// waited for, with two exceptions that steady state does not meet: a block or an arena that has to grow, and a call issued
// while the upload of the call before it has not yet left the staging block.
static bool track_frames(OrbxTrackFrames &F, const orbx_keypoint *d_keys_un, const uint8_t *d_desc, const float *d_u_right,
                         const int32_t *d_counts, int cap, const int32_t *d_cell_begin, const uint16_t *d_items, const float *bounds4) {
    if (!grid_params(bounds4[0], bounds4[1], bounds4[2], bounds4[3], F.gp)) return false;
    for (int i = 0; i < 4; ++i) F.bounds[i] = bounds4[i];
    F.kps = d_keys_un; F.desc = d_desc; F.ur = d_u_right; F.counts = d_counts; F.cap = cap;
    F.cell_begin = d_cell_begin; F.items = d_items;
    return true;
}

extern "C" orbx_status orbx_search_by_projection_frame_batch_device(orbx_handle *h, int nproblems, const orbx_track_frame_problem *problems,
                                                                    int nframes, const orbx_keypoint *d_keys_un, const uint8_t *d_desc,
                                                                    const float *d_u_right, const int32_t *d_counts, int cap,
                                                                    const int32_t *d_cell_begin, const uint16_t *d_items,
                                                                    const float *camera4, const float *bounds4, float mb, float mbf,
                                                                    int check_orientation, int32_t *d_matched_last, int32_t *d_nmatches) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    const OrbxTrackBatchArgs a = {nframes, cap, h->p.nlevels,
                                  nproblems <= 0 || (d_keys_un && d_desc && d_counts && d_cell_begin && d_items && camera4 && bounds4 &&
                                                     d_matched_last && d_nmatches)};
    OrbxTrackPlan plan;
    const char *why = "";
    orbx_status st = orbx_track_frame_plan(nproblems, problems, a, plan, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    OrbxTrackFrames F;
    if (nproblems > 0 && !track_frames(F, d_keys_un, d_desc, d_u_right, d_counts, cap, d_cell_begin, d_items, bounds4))
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad image bounds");
    if (nproblems == 0) return ORBX_OK;
    if (h->host_only) return orbx_fail(ORBX_NO_DEVICE, "no device handle");
    uint8_t *pin = nullptr, *d = nullptr;
    st = stage_begin(h, plan.in_bytes, plan.dev_bytes, &pin, &d, true);
    if (st != ORBX_OK) return st;
    orbx_track_frame_pack(nproblems, problems, plan, h->tab.scale, mb, pin);
    st = stage_upload(h, pin, d, plan.in_bytes);
    if (st != ORBX_OK) return st;
    const DTrackProb *dp = (const DTrackProb *)(d + plan.o_prob);
    DTrackQ *dq = (DTrackQ *)(d + plan.o_q);
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_track_project(h->stream, F, camera4, mbf, h->p.fp_mode == ORBX_FP_GCC_FMA ? 1 : 0, dp, dq, (int)plan.nq); }
    { ProfScope ps(h, ORBX_K_MATCH);
      orbx_launch_track_cand(h->stream, false, F, dp, dq, d + plan.o_desc, (int)plan.nq, (uint4 *)(d + plan.o_cand)); }
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_track_select(h->stream, false, F, nproblems, dp, dq, d + plan.o_desc, (const uint4 *)(d + plan.o_cand), nullptr, 0.f,
                               check_orientation ? 1 : 0, (int32_t *)(d + plan.o_ev), d_matched_last, d_nmatches); }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    return ORBX_OK;
}

extern "C" orbx_status orbx_search_by_projection_mappoints_batch_device(orbx_handle *h, int nproblems,
                                                                        const orbx_track_points_problem *problems, int nframes,
                                                                        const orbx_keypoint *d_keys_un, const uint8_t *d_desc,
                                                                        const float *d_u_right, const int32_t *d_counts, int cap,
                                                                        const int32_t *d_cell_begin, const uint16_t *d_items,
                                                                        const float *bounds4, float nnratio, int32_t *d_assigned,
                                                                        int32_t *d_nmatches) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    const OrbxTrackBatchArgs a = {nframes, cap, h->p.nlevels,
                                  nproblems <= 0 || (d_keys_un && d_desc && d_counts && d_cell_begin && d_items && bounds4 && d_assigned &&
                                                     d_nmatches)};
    OrbxTrackPlan plan;
    const char *why = "";
    orbx_status st = orbx_track_points_plan(nproblems, problems, a, plan, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    OrbxTrackFrames F;
    if (nproblems > 0 && !track_frames(F, d_keys_un, d_desc, d_u_right, d_counts, cap, d_cell_begin, d_items, bounds4))
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad image bounds");
    if (nproblems == 0) return ORBX_OK;
    if (h->host_only) return orbx_fail(ORBX_NO_DEVICE, "no device handle");
    uint8_t *pin = nullptr, *d = nullptr;
    st = stage_begin(h, plan.in_bytes, plan.dev_bytes, &pin, &d, true);
    if (st != ORBX_OK) return st;
    orbx_track_points_pack(nproblems, problems, plan, h->tab.scale, cap, pin);
    st = stage_upload(h, pin, d, plan.in_bytes);
    if (st != ORBX_OK) return st;
    const DTrackProb *dp = (const DTrackProb *)(d + plan.o_prob);
    const DTrackQ *dq = (const DTrackQ *)(d + plan.o_q);
    { ProfScope ps(h, ORBX_K_MATCH);
      orbx_launch_track_cand(h->stream, true, F, dp, dq, d + plan.o_desc, (int)plan.nq, (uint4 *)(d + plan.o_cand)); }
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_track_select(h->stream, true, F, nproblems, dp, dq, d + plan.o_desc, (const uint4 *)(d + plan.o_cand),
                               (const uint32_t *)(d + plan.o_seed), nnratio, 0, (int32_t *)(d + plan.o_ev), d_assigned, d_nmatches); }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    return ORBX_OK;
}

// ---------------------------------------------------------------- MapPoint::PredictScale (host; works on a host-only handle)
extern "C" orbx_status orbx_predict_scale_table(const orbx_handle *h, float *thr, int n) {
    if (!h || !thr) return orbx_fail(ORBX_BAD_ARGUMENT, "null argument");
    if (n < h->p.nlevels) return orbx_fail(ORBX_BAD_ARGUMENT, "n < nlevels");
    memcpy(thr, h->ps_thr, (size_t)h->p.nlevels * sizeof(float));
    return ORBX_OK;
}
extern "C" int orbx_predict_scale(const orbx_handle *h, float max_distance, float current_dist) {
    if (!h) return -1;
    return orbx_predict_scale_level(h->ps_thr, h->p.nlevels, max_distance / current_dist);
}

// ---------------------------------------------------------------- Tracking::SearchLocalPoints, batched and device-resident:
// k_track_frustum (isInFrustum + PredictScale + the matcher's window, one thread per (problem, point), the pool's descriptors
// gathered per query) in front of the k_track_cand + k_track_select of the map-point policy, which run as they are.
extern "C" orbx_status orbx_search_local_points_batch_device(orbx_handle *h, int nproblems, const orbx_track_local_problem *problems,
                                                             const orbx_local_map_view *map, int nframes,
                                                             const orbx_keypoint *d_keys_un, const uint8_t *d_desc,
                                                             const float *d_u_right, const int32_t *d_counts, int cap,
                                                             const int32_t *d_cell_begin, const uint16_t *d_items,
                                                             const float *camera4, const float *bounds4, float mbf, float nnratio,
                                                             int32_t *d_assigned, int32_t *d_nmatches, uint8_t *d_in_view,
                                                             orbx_track_state *d_track) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "no handle");
    const OrbxTrackBatchArgs a = {nframes, cap, h->p.nlevels,
                                  nproblems <= 0 || (d_keys_un && d_desc && d_counts && d_cell_begin && d_items && camera4 && bounds4 &&
                                                     d_assigned && d_nmatches)};
    OrbxLocalPlan plan;
    const char *why = "";
    orbx_status st = orbx_track_local_plan(nproblems, problems, map, a, plan, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    OrbxTrackFrames F;
    if (nproblems > 0 && !track_frames(F, d_keys_un, d_desc, d_u_right, d_counts, cap, d_cell_begin, d_items, bounds4))
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad image bounds");
    if (nproblems == 0) return ORBX_OK;
    if (h->host_only) return orbx_fail(ORBX_NO_DEVICE, "no device handle");
    uint8_t *pin = nullptr, *d = nullptr;
    st = stage_begin(h, plan.in_bytes, plan.dev_bytes, &pin, &d, true);
    if (st != ORBX_OK) return st;
    orbx_track_local_pack(nproblems, problems, map, plan, cap, pin);
    st = stage_upload(h, pin, d, plan.in_bytes);
    if (st != ORBX_OK) return st;
    const DTrackProb *dp = (const DTrackProb *)(d + plan.o_prob);
    DTrackQ *dq = (DTrackQ *)(d + plan.o_q);
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_track_frustum(h->stream, F, camera4, mbf, h->p.fp_mode == ORBX_FP_GCC_FMA ? 1 : 0, h->p.nlevels, h->ps_thr,
                                h->tab.scale, nproblems, plan.max_points, dp, (const DTrackLocal *)(d + plan.o_local),
                                (const DTrackPoolPt *)(d + plan.o_pool), d + plan.o_pdesc, (const int32_t *)(d + plan.o_index),
                                d + plan.o_skip, dq, d + plan.o_desc, d_in_view, d_track); }
    { ProfScope ps(h, ORBX_K_MATCH);
      orbx_launch_track_cand(h->stream, true, F, dp, dq, d + plan.o_desc, (int)plan.nq, (uint4 *)(d + plan.o_cand)); }
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_track_select(h->stream, true, F, nproblems, dp, dq, d + plan.o_desc, (const uint4 *)(d + plan.o_cand),
                               (const uint32_t *)(d + plan.o_seed), nnratio, 0, (int32_t *)(d + plan.o_ev), d_assigned, d_nmatches); }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    return ORBX_OK;
}
