// orbx_match.cpp -- matching behind the C ABI: the device grid and the gated candidate lists (orbx_gate.h, shared with
// orbx_tracking.cpp and orbx_policies.cpp), brute-force matching and the Hamming matrix, and the host-side policies on top:
// the Frame grid, ComputeThreeMaxima and SearchForInitialization.
#include <climits>
#include <cmath>
#include <cstring>
#include <algorithm>
#include <vector>
#include "orbx_handle.h"
#include "orbx_gate.h"

// ---------------------------------------------------------------- device grid + gated candidate lists (orbx_gate.h)
static orbx_status gate_items_reserve(orbx_handle *h, size_t words) {
    return dev_grow(h, (void **)&h->d_gate_items, &h->gate_items_cap, words, std::max(words + words / 2, (size_t)1 << 16), sizeof(uint32_t));
}

// Frame::AssignFeaturesToGrid on the device, for the buffers orbx_extract_batch_device (or orbx_undistort_keypoints_device)
// filled: the keypoints never leave the GPU between extraction and a gated match.
extern "C" orbx_status orbx_grid_build_device(orbx_handle *h, int nframes, const orbx_keypoint *d_kps, const int32_t *d_counts,
                                              int cap, const float *bounds4, int32_t *d_cell_begin, uint16_t *d_items) {
    if (!h || h->host_only) return orbx_fail(h ? ORBX_NO_DEVICE : ORBX_BAD_ARGUMENT, "no device handle");
    if (nframes <= 0 || !d_kps || !d_counts || cap <= 0 || cap > 65535 || !bounds4 || !d_cell_begin || !d_items)
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument (cap <= 65535: bucket entries are 16-bit feature indices)");
    DGrid gp;
    if (!grid_params(bounds4[0], bounds4[1], bounds4[2], bounds4[3], gp)) return orbx_fail(ORBX_BAD_ARGUMENT, "bad image bounds");
    HIPCHK(hipSetDevice(h->dev));
    { ProfScope ps(h, ORBX_K_MISC);
      orbx_launch_grid_build(h->stream, gp, nframes, d_kps, d_counts, 0, cap, d_cell_begin, d_items); }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    return ORBX_OK;
}

// One call = one upload (everything packed into page-locked staging), two kernels (k_grid_build, k_gate) and one download that
// is waited for: the (offset, count) spans, the fill count, and speculatively as many candidate entries as the last call
// produced (+50 %) -- only a call that produces more than that pays a second copy.
// BATCHED: K targets (keyframes) share the call -- their keypoints / descriptors are packed `fstride` records apart, k_grid_build
// builds the K grids in one launch (one workgroup per target), every query names its target (DGateQuery::frame) and k_gate
// serves all of them in one launch.  The ~60 us floor of a synchronous call (upload, two launches, waited download) is paid once
// per batch instead of once per (keyframe, point set) pair.  All targets share the image bounds (Frame's static mnMinX .. mnMaxY).
orbx_status orbx_gate_lists_batch(orbx_handle *h, const OrbxGateTarget *tg, int K, float min_x, float max_x, float min_y, float max_y,
                                  const DGateQuery *q, const uint8_t *qdesc, int nq, OrbxGateLists &out, int nqdesc) {
    if (nqdesc < 0) nqdesc = nq;
    out.span.assign((size_t)std::max(nq, 0), make_uint2(0u, 0u));
    out.items.clear();
    if (!h || h->host_only) return orbx_fail(h ? ORBX_NO_DEVICE : ORBX_BAD_ARGUMENT, "no device handle");
    int fstride = 0;
    for (int k = 0; k < K; ++k) fstride = std::max(fstride, tg[k].n);
    if (nq <= 0 || K <= 0 || fstride <= 0) return ORBX_OK;
    if (fstride > 65535) return orbx_fail(ORBX_UNSUPPORTED, "more than 65535 target features (candidate entries carry 16-bit indices)");
    DGrid gp;
    if (!grid_params(min_x, max_x, min_y, max_y, gp)) return orbx_fail(ORBX_BAD_ARGUMENT, "bad image bounds");
    HIPCHK(hipSetDevice(h->dev));
    const size_t nrec = (size_t)K * fstride;
    // input block (uploaded in one copy): cursor | counts | keys | descriptors | queries | query descriptors
    const size_t o_cur = 0, o_cnt = 256, o_keys = o_cnt + pad256((size_t)K * sizeof(int)), o_desc = o_keys + pad256(nrec * sizeof(orbx_keypoint)),
                 o_q = o_desc + pad256(nrec * 32), o_qd = o_q + pad256((size_t)nq * sizeof(DGateQuery)), in_bytes = o_qd + pad256((size_t)nqdesc * 32);
    // device-only: bucket offsets | bucket items | spans
    const size_t o_cb = in_bytes, o_it = o_cb + pad256((size_t)K * (64 * 48 + 1) * sizeof(int)), o_span = o_it + pad256(nrec * sizeof(uint16_t)),
                 dev_bytes = o_span + pad256((size_t)nq * sizeof(uint2));
    orbx_status st = scratch_reserve(h, dev_bytes + 256);
    if (st != ORBX_OK) return st;
    st = gate_items_reserve(h, std::max(h->gate_guess, (size_t)1 << 16));
    if (st != ORBX_OK) return st;
    const size_t span_bytes = (size_t)nq * sizeof(uint2);
    size_t guess = std::min(h->gate_guess, h->gate_items_cap);
    st = stage_pin(h, in_bytes + span_bytes + 256 + h->gate_items_cap * 4);   // (sized by the candidate buffer, which may grow again below)
    if (st != ORBX_OK) return st;
    uint8_t *pin_in = h->pin, *pin_out = h->pin + in_bytes;   // pin_out: spans | cursor (256) | items
    memset(pin_in + o_cur, 0, 256);
    for (int k = 0; k < K; ++k) {
        ((int *)(pin_in + o_cnt))[k] = tg[k].n;
        if (tg[k].n <= 0) continue;
        memcpy(pin_in + o_keys + (size_t)k * fstride * sizeof(orbx_keypoint), tg[k].keys, (size_t)tg[k].n * sizeof(orbx_keypoint));
        memcpy(pin_in + o_desc + (size_t)k * fstride * 32, tg[k].desc, (size_t)tg[k].n * 32);
    }
    memcpy(pin_in + o_q, q, (size_t)nq * sizeof(DGateQuery));
    memcpy(pin_in + o_qd, qdesc, (size_t)nqdesc * 32);
    uint8_t *d = scratch_take<uint8_t>(h, dev_bytes);
    uint32_t *dcur = (uint32_t *)(d + o_cur);
    const orbx_keypoint *dk = (const orbx_keypoint *)(d + o_keys);
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(d, pin_in, in_bytes, hipMemcpyHostToDevice, s));
    uint32_t total = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        { ProfScope ps(h, ORBX_K_MATCH);
          if (attempt == 0) orbx_launch_grid_build(s, gp, K, dk, (const int *)(d + o_cnt), 0, fstride, (int *)(d + o_cb), (uint16_t *)(d + o_it));
          orbx_launch_gate(s, gp, dk, d + o_desc, (const int *)(d + o_cb), (const uint16_t *)(d + o_it), (const DGateQuery *)(d + o_q),
                           d + o_qd, nq, (uint2 *)(d + o_span), dcur, h->d_gate_items, (uint32_t)std::min<size_t>(h->gate_items_cap, 0xffffffffu),
                           fstride); }
        HIPCHK(hipMemcpyAsync(pin_out, d + o_span, span_bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(pin_out + span_bytes, dcur, 4, hipMemcpyDeviceToHost, s));
        if (guess > 0) HIPCHK(hipMemcpyAsync(pin_out + span_bytes + 256, h->d_gate_items, guess * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        memcpy(&total, pin_out + span_bytes, 4);
        if (total <= h->gate_items_cap) break;
        // the lists did not fit the buffer: nothing beyond the spans was trusted; grow, reset the cursor, run k_gate again
        if (attempt == 1) return orbx_fail(ORBX_CAPACITY, "candidate lists");
        st = gate_items_reserve(h, total);
        if (st == ORBX_OK) st = stage_pin(h, in_bytes + span_bytes + 256 + h->gate_items_cap * 4);
        if (st != ORBX_OK) return st;
        pin_in = h->pin; pin_out = h->pin + in_bytes;
        HIPCHK(hipMemsetAsync(dcur, 0, 4, s));
        guess = total;
    }
    if (total > guess) {   // more entries than the speculative copy covered
        HIPCHK(hipMemcpyAsync(pin_out + span_bytes + 256 + guess * 4, h->d_gate_items + guess, (size_t)(total - guess) * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    h->gate_guess = std::max<size_t>(4096, (size_t)total + total / 2);
    memcpy(out.span.data(), pin_out, span_bytes);
    out.items.resize(total);
    if (total) memcpy(out.items.data(), pin_out + span_bytes + 256, (size_t)total * 4);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    return ORBX_OK;
}
orbx_status orbx_gate_lists(orbx_handle *h, const orbx_keypoint *tkeys, const uint8_t *tdesc, int nt, float min_x, float max_x,
                            float min_y, float max_y, const DGateQuery *q, const uint8_t *qdesc, int nq, OrbxGateLists &out) {
    const OrbxGateTarget tg = {tkeys, tdesc, nt};
    return orbx_gate_lists_batch(h, &tg, 1, min_x, max_x, min_y, max_y, q, qdesc, nq, out);
}

// host-buffer form of the primitive itself (tests, tools/policy_rates.py): xyr = (x, y, r) per query, levels = (min, max)
extern "C" orbx_status orbx_gated_candidates(orbx_handle *h, const orbx_keypoint *tkeys, const uint8_t *tdesc, int nt,
                                             const float *bounds4, const float *xyr, const int32_t *levels, const uint8_t *qdesc,
                                             int nq, uint32_t *begin, uint32_t *items, int items_cap, int *total) {
    if (!h || !bounds4 || nq < 0 || nt < 0 || !begin || !total || (nq > 0 && (!xyr || !levels || !qdesc)) || (nt > 0 && (!tkeys || !tdesc)))
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    std::vector<DGateQuery> q((size_t)nq);
    for (int i = 0; i < nq; ++i) { q[i].x = xyr[3 * i]; q[i].y = xyr[3 * i + 1]; q[i].r = xyr[3 * i + 2]; q[i].min_level = levels[2 * i]; q[i].max_level = levels[2 * i + 1]; }
    OrbxGateLists L;
    orbx_status st = orbx_gate_lists(h, tkeys, tdesc, nt, bounds4[0], bounds4[1], bounds4[2], bounds4[3], q.data(), qdesc, nq, L);
    if (st != ORBX_OK) return st;
    begin[0] = 0;
    for (int i = 0; i < nq; ++i) begin[i + 1] = begin[i] + (uint32_t)L.count(i);
    *total = (int)begin[nq];
    if ((int)begin[nq] > items_cap) return orbx_fail(ORBX_CAPACITY, "candidate list capacity");
    for (int i = 0; i < nq && items; ++i)
        if (L.count(i)) memcpy(items + begin[i], L.list(i), (size_t)L.count(i) * 4);
    return ORBX_OK;
}

orbx_status orbx_block_distances(orbx_handle *h, const uint8_t *d1, int n1, const uint8_t *d2, int n2,
                                 const std::vector<DDistRow> &rows, const std::vector<uint32_t> &col_idx, size_t total,
                                 std::vector<uint16_t> &out) {
    out.assign(total, 0);
    if (!h || h->host_only) return orbx_fail(h ? ORBX_NO_DEVICE : ORBX_BAD_ARGUMENT, "no device handle");
    if (rows.empty() || total == 0) return ORBX_OK;
    const size_t o_a = 0, o_b = o_a + pad256((size_t)n1 * 32), o_r = o_b + pad256((size_t)n2 * 32),
                 o_c = o_r + pad256(rows.size() * sizeof(DDistRow)), in_bytes = o_c + pad256(col_idx.size() * 4);
    uint8_t *pin_in = nullptr, *d = nullptr;
    orbx_status st = stage_begin(h, in_bytes + pad256(total * sizeof(uint16_t)), in_bytes, &pin_in, &d, false);
    if (st == ORBX_OK) st = gate_items_reserve(h, (total + 1) / 2);
    if (st != ORBX_OK) return st;
    uint8_t *pin_out = pin_in + in_bytes;
    memcpy(pin_in + o_a, d1, (size_t)n1 * 32);
    memcpy(pin_in + o_b, d2, (size_t)n2 * 32);
    memcpy(pin_in + o_r, rows.data(), rows.size() * sizeof(DDistRow));
    memcpy(pin_in + o_c, col_idx.data(), col_idx.size() * 4);
    st = stage_upload(h, pin_in, d, in_bytes);
    if (st != ORBX_OK) return st;
    { ProfScope ps(h, ORBX_K_MATCH);
      orbx_launch_block_dist(h->stream, d + o_a, d + o_b, (const DDistRow *)(d + o_r), (const uint32_t *)(d + o_c), (int)rows.size(),
                             (uint16_t *)h->d_gate_items); }
    st = stage_download_wait(h, pin_out, (const uint8_t *)h->d_gate_items, total * sizeof(uint16_t));
    if (st != ORBX_OK) return st;
    memcpy(out.data(), pin_out, total * sizeof(uint16_t));
    return ORBX_OK;
}

// Batched SearchByBoW: one upload (every set's descriptors, angles, MapPoint flags and feature-vector indices, the work list,
// the outputs preset to -1), k_bow_select + k_bow_rot, one download of the outputs and counts, one synchronisation.
orbx_status orbx_bow_select_batch(orbx_handle *h, bool kk, const OrbxBowSet *sets, int nsets, const std::vector<DBowItem> &items,
                                  int max_ncol, float nnratio, int check_orientation, int32_t *const *outs, int *nmatches) {
    if (!h || h->host_only) return orbx_fail(h ? ORBX_NO_DEVICE : ORBX_BAD_ARGUMENT, "no device handle");
    const int K = nsets - 1, nout = sets[0].n;
    size_t nfeat = 0, nidx = 0;
    for (int s = 0; s < nsets; ++s) {
        nfeat += (size_t)sets[s].n;
        nidx += sets[s].fv->n_nodes > 0 ? (size_t)sets[s].fv->begin[sets[s].fv->n_nodes] : 0;
    }
    if (nfeat > 0xffffffffull / 32 || nidx > 0xffffffffull || (size_t)K * nout > 0xffffffffull)
        return orbx_fail(ORBX_UNSUPPORTED, "batch too large for 32-bit offsets");
    // counts | outputs (the download) | descriptors | angles | MapPoint flags | indices | work items | candidate bases
    const size_t o_cnt = 0, o_out = pad256((size_t)K * 4), o_desc = o_out + pad256((size_t)K * nout * 4),
                 o_ang = o_desc + pad256(nfeat * 32), o_hmp = o_ang + pad256(nfeat * 4), o_idx = o_hmp + pad256(nfeat),
                 o_it = o_idx + pad256(nidx * 4), o_cb = o_it + pad256(items.size() * sizeof(DBowItem)),
                 in_bytes = o_cb + pad256((size_t)K * 4), down_bytes = o_out + (size_t)K * nout * 4;
    uint8_t *pin = nullptr, *d = nullptr;
    orbx_status st = stage_begin(h, in_bytes, in_bytes, &pin, &d, false);
    if (st != ORBX_OK) return st;
    memset(pin + o_cnt, 0, (size_t)K * 4);
    memset(pin + o_out, 0xff, (size_t)K * nout * 4);
    size_t fb = 0, ib = 0;
    for (int s = 0; s < nsets; ++s) {
        const OrbxBowSet &S = sets[s];
        if (s > 0) ((uint32_t *)(pin + o_cb))[s - 1] = (uint32_t)fb;
        if (S.n > 0) {
            memcpy(pin + o_desc + fb * 32, S.desc, (size_t)S.n * 32);
            float *ang = (float *)(pin + o_ang) + fb;
            for (int i = 0; i < S.n; ++i) ang[i] = S.keys[i].angle;
            if (S.hmp) memcpy(pin + o_hmp + fb, S.hmp, (size_t)S.n);
            else memset(pin + o_hmp + fb, 0, (size_t)S.n);
        }
        const size_t ni = S.fv->n_nodes > 0 ? (size_t)S.fv->begin[S.fv->n_nodes] : 0;
        if (ni) memcpy(pin + o_idx + ib * 4, S.fv->index, ni * 4);
        fb += (size_t)S.n; ib += ni;
    }
    if (!items.empty()) memcpy(pin + o_it, items.data(), items.size() * sizeof(DBowItem));
    hipStream_t s = h->stream;
    st = stage_upload(h, pin, d, in_bytes);
    if (st != ORBX_OK) return st;
    { ProfScope ps(h, ORBX_K_MATCH);
      orbx_launch_bow_select(s, kk, (const DBowItem *)(d + o_it), (int)items.size(), (const uint32_t *)(d + o_idx), d + o_desc,
                             d + o_hmp, nnratio, std::max(1, (max_ncol + 31) / 32), (int32_t *)(d + o_out));
      orbx_launch_bow_rot(s, kk, K, nout, (const uint32_t *)(d + o_cb), (const float *)(d + o_ang), check_orientation ? 1 : 0,
                          (int32_t *)(d + o_out), (int32_t *)(d + o_cnt)); }
    st = stage_download_wait(h, pin, d, down_bytes);
    if (st != ORBX_OK) return st;
    for (int k = 0; k < K; ++k) {
        nmatches[k] = ((const int32_t *)(pin + o_cnt))[k];
        if (nout > 0) memcpy(outs[k], pin + o_out + (size_t)k * nout * 4, (size_t)nout * 4);
    }
    return ORBX_OK;
}

// ---------------------------------------------------------------- matching
extern "C" orbx_status orbx_match_bruteforce_device(orbx_handle *h, int npairs, const uint8_t *d_q, const int32_t *d_nq,
                                                    int64_t q_stride, const uint8_t *d_t, const int32_t *d_nt,
                                                    int64_t t_stride, int32_t *d_best_idx, int32_t *d_best_dist,
                                                    int32_t *d_second_dist, int out_stride) {
    if (!h || h->host_only) return orbx_fail(h ? ORBX_NO_DEVICE : ORBX_BAD_ARGUMENT, "no device handle");
    if (npairs <= 0 || !d_q || !d_t || !d_nq || !d_nt || !d_best_idx || !d_best_dist || !d_second_dist || out_stride <= 0)
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    HIPCHK(hipSetDevice(h->dev));
    const size_t need = orbx_match_workspace_bytes(npairs, out_stride);
    const orbx_status st = dev_grow(h, &h->d_match_ws, &h->match_ws_bytes, need, need);   // grows only when a larger problem than ever before arrives
    if (st != ORBX_OK) return st;
    { ProfScope ps(h, ORBX_K_MATCH);
      orbx_launch_match(h->stream, npairs, out_stride, d_q, d_nq, q_stride, d_t, d_nt, t_stride, d_best_idx, d_best_dist,
                        d_second_dist, out_stride, h->d_match_ws, h->match_kernel); }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    return ORBX_OK;
}

extern "C" orbx_status orbx_match_bruteforce(orbx_handle *h, const uint8_t *q, int nq, const uint8_t *t, int nt,
                                             int32_t *best_idx, int32_t *best_dist, int32_t *second_dist) {
    if (!h || h->host_only) return orbx_fail(h ? ORBX_NO_DEVICE : ORBX_BAD_ARGUMENT, "no device handle");
    if (nq < 0 || nt < 0 || (nq > 0 && (!q || !best_idx || !best_dist || !second_dist)) || (nt > 0 && !t))
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    if (nq == 0) return ORBX_OK;
    HIPCHK(hipSetDevice(h->dev));
    orbx_status st = scratch_reserve(h, pad256((size_t)nq * 32) + pad256((size_t)std::max(nt, 1) * 32) + 256 +
                                            pad256((size_t)3 * nq * sizeof(int)));
    if (st != ORBX_OK) return st;
    uint8_t *dq = scratch_take<uint8_t>(h, (size_t)nq * 32), *dt = scratch_take<uint8_t>(h, (size_t)std::max(nt, 1) * 32);
    int *dn = scratch_take<int>(h, 2), *dout = scratch_take<int>(h, (size_t)3 * nq);
    int hn[2] = {nq, nt};
    HIPCHK(hipMemcpyAsync(dq, q, (size_t)nq * 32, hipMemcpyHostToDevice, h->stream));
    if (nt > 0) HIPCHK(hipMemcpyAsync(dt, t, (size_t)nt * 32, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dn, hn, sizeof(hn), hipMemcpyHostToDevice, h->stream));
    st = orbx_match_bruteforce_device(h, 1, dq, dn, 0, dt, dn + 1, 0, dout, dout + nq, dout + 2 * nq, nq);
    if (st == ORBX_OK) {
        HIPCHK(hipMemcpyAsync(best_idx, dout, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(best_dist, dout + nq, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(second_dist, dout + 2 * nq, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));   // also keeps hn[] alive until the H2D copy has been consumed
    }
    return st;
}

extern "C" orbx_status orbx_hamming_matrix(orbx_handle *h, const uint8_t *q, int nq, const uint8_t *t, int nt,
                                           uint16_t *dist) {
    if (!h || h->host_only) return orbx_fail(h ? ORBX_NO_DEVICE : ORBX_BAD_ARGUMENT, "no device handle");
    if (nq <= 0 || nt <= 0) return ORBX_OK;
    if (!q || !t || !dist) return orbx_fail(ORBX_BAD_ARGUMENT, "null argument");
    HIPCHK(hipSetDevice(h->dev));
    orbx_status st = scratch_reserve(h, pad256((size_t)nq * 32) + pad256((size_t)nt * 32) + pad256((size_t)nq * nt * sizeof(uint16_t)));
    if (st != ORBX_OK) return st;
    uint8_t *dq = scratch_take<uint8_t>(h, (size_t)nq * 32), *dt = scratch_take<uint8_t>(h, (size_t)nt * 32);
    uint16_t *dd = scratch_take<uint16_t>(h, (size_t)nq * nt);
    HIPCHK(hipMemcpyAsync(dq, q, (size_t)nq * 32, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dt, t, (size_t)nt * 32, hipMemcpyHostToDevice, h->stream));
    { ProfScope ps(h, ORBX_K_MATCH);
      orbx_launch_hamming_matrix(h->stream, dq, nq, dt, nt, dd); }
    hipError_t e = hipMemcpyAsync(dist, dd, (size_t)nq * nt * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    return ORBX_OK;
}

// ================================================================ matcher policies on the path (a13, a16, a17)
// The Hamming work runs on the GPU; the order-dependent bookkeeping of each policy is host code, as the
// reference's own structure dictates.

// ---------------------------------------------------------------- a17: Frame grid (src/Frame.cc:432-460, 633-745)
struct orbx_grid {
    static const int COLS = 64, ROWS = 48;     // FRAME_GRID_COLS / FRAME_GRID_ROWS (include/Frame.h:54,59)
    float minx, miny, winv, hinv;
    const orbx_keypoint *kps;
    std::vector<int> begin, items;
};

extern "C" orbx_grid *orbx_grid_create(const orbx_keypoint *kps, int n, float min_x, float max_x, float min_y, float max_y) {
    if (n < 0 || (n > 0 && !kps) || !(max_x > min_x) || !(max_y > min_y)) { orbx_fail(ORBX_BAD_ARGUMENT, "bad grid arguments"); return nullptr; }
    orbx_grid *g = new orbx_grid();
    g->minx = min_x; g->miny = min_y; g->kps = kps;
    g->winv = (float)orbx_grid::COLS / (max_x - min_x);
    g->hinv = (float)orbx_grid::ROWS / (max_y - min_y);
    const int nc = orbx_grid::COLS * orbx_grid::ROWS;
    std::vector<int> cell(n);
    g->begin.assign(nc + 1, 0);
    for (int i = 0; i < n; ++i) {                     // PosInGrid: C round(), then the range test
        const int px = (int)roundf((kps[i].x - min_x) * g->winv), py = (int)roundf((kps[i].y - min_y) * g->hinv);
        cell[i] = (px < 0 || px >= orbx_grid::COLS || py < 0 || py >= orbx_grid::ROWS) ? -1 : px * orbx_grid::ROWS + py;
        if (cell[i] >= 0) g->begin[cell[i] + 1]++;
    }
    for (int c = 0; c < nc; ++c) g->begin[c + 1] += g->begin[c];
    g->items.resize(n);
    std::vector<int> fill(nc, 0);
    for (int i = 0; i < n; ++i)
        if (cell[i] >= 0) g->items[g->begin[cell[i]] + fill[cell[i]]++] = i;   // push_back order = feature order
    return g;
}
extern "C" void orbx_grid_destroy(orbx_grid *g) { delete g; }

// GetFeaturesInArea: same cell walk (x outer, y inner), same level filter quirk (`minLevel > 0 || maxLevel >= 0`)
extern "C" int orbx_grid_query(const orbx_grid *g, float x, float y, float r, int min_level, int max_level, int32_t *out,
                               int cap) {
    if (!g) return -1;
    int x0 = std::max(0, (int)floorf((x - g->minx - r) * g->winv));
    if (x0 >= orbx_grid::COLS) return 0;
    int x1 = std::min(orbx_grid::COLS - 1, (int)ceilf((x - g->minx + r) * g->winv));
    if (x1 < 0) return 0;
    int y0 = std::max(0, (int)floorf((y - g->miny - r) * g->hinv));
    if (y0 >= orbx_grid::ROWS) return 0;
    int y1 = std::min(orbx_grid::ROWS - 1, (int)ceilf((y - g->miny + r) * g->hinv));
    if (y1 < 0) return 0;
    const bool check = (min_level > 0) || (max_level >= 0);
    int n = 0;
    for (int ix = x0; ix <= x1; ++ix)
        for (int iy = y0; iy <= y1; ++iy) {
            const int c = ix * orbx_grid::ROWS + iy;
            for (int j = g->begin[c]; j < g->begin[c + 1]; ++j) {
                const orbx_keypoint &kp = g->kps[g->items[j]];
                if (check) {
                    if (kp.octave < min_level) continue;
                    if (max_level >= 0 && kp.octave > max_level) continue;
                }
                if (fabsf(kp.x - x) < r && fabsf(kp.y - y) < r) {
                    if (n < cap && out) out[n] = g->items[j];
                    ++n;
                }
            }
        }
    return n;
}

// ---------------------------------------------------------------- a15: ComputeThreeMaxima (src/ORBmatcher.cc:2026-2068)
extern "C" void orbx_three_maxima(const int32_t *sizes, int L, int *ind1, int *ind2, int *ind3) {
    int max1 = 0, max2 = 0, max3 = 0;
    *ind1 = *ind2 = *ind3 = -1;
    for (int i = 0; i < L; ++i) {
        const int s = sizes[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; *ind3 = *ind2; *ind2 = *ind1; *ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; *ind3 = *ind2; *ind2 = i; }
        else if (s > max3) { max3 = s; *ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { *ind2 = -1; *ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { *ind3 = -1; }
}

// ---------------------------------------------------------------- a13: SearchForInitialization (src/ORBmatcher.cc:570-712)
// GPU: the grid of F2 and, per level-0 feature of F1, its window's candidates with their Hamming distances in the
// reference's visiting order (orbx_gate_lists).  Host: the sequential selection pass over those lists.
extern "C" orbx_status orbx_search_for_initialization(orbx_handle *h, const orbx_keypoint *k1, const uint8_t *d1, int n1,
                                                      const orbx_keypoint *k2, const uint8_t *d2, int n2,
                                                      const float *bounds4, float *prev_matched, int window,
                                                      float nnratio, int check_orientation, int32_t *matches12,
                                                      int *nmatches_out) {
    if (!h || h->host_only) return orbx_fail(h ? ORBX_NO_DEVICE : ORBX_BAD_ARGUMENT, "no device handle");
    if (n1 < 0 || n2 < 0 || !bounds4 || !matches12 || !nmatches_out || (n1 > 0 && (!k1 || !d1 || !prev_matched)) ||
        (n2 > 0 && (!k2 || !d2)))
        return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    const int HISTO = 30, TH_LOW_ = 50;
    *nmatches_out = 0;
    for (int i = 0; i < n1; ++i) matches12[i] = -1;
    if (n1 == 0 || n2 == 0) return ORBX_OK;
    // GPU: GetFeaturesInArea(vbPrevMatched[i1], windowSize, level1, level1) + DescriptorDistance for every level-0 feature
    // of F1, as ordered candidate lists (k_grid_build + k_gate); features of other levels never reach the loop (:603-605)
    std::vector<DGateQuery> gq((size_t)n1);
    for (int i1 = 0; i1 < n1; ++i1) {
        const int level1 = k1[i1].octave;
        gq[i1].x = prev_matched[2 * i1]; gq[i1].y = prev_matched[2 * i1 + 1];
        gq[i1].r = level1 > 0 ? -1.0f : (float)window;
        gq[i1].min_level = level1; gq[i1].max_level = level1;
    }
    OrbxGateLists gl;
    { const orbx_status st = orbx_gate_lists(h, k2, d2, n2, bounds4[0], bounds4[1], bounds4[2], bounds4[3], gq.data(), d1, n1, gl);
      if (st != ORBX_OK) return st; }
    int nmatches = 0;
    std::vector<std::vector<int>> rotHist(HISTO);
    const float factor = HISTO / 360.0f;               // fork value (src/ORBmatcher.cc:583)
    std::vector<int> matchedDist(n2, INT_MAX), matches21(n2, -1);
    for (int i1 = 0; i1 < n1; ++i1) {
        const int level1 = k1[i1].octave;
        if (level1 > 0) continue;
        const int nc = gl.count(i1);
        if (nc == 0) continue;
        const uint32_t *cl = gl.list(i1);
        int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
        for (int c = 0; c < nc; ++c) {
            const int i2 = OrbxGateLists::idx(cl[c]), dist = OrbxGateLists::dist(cl[c]);
            if (matchedDist[i2] <= dist) continue;
            if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx2 = i2; }
            else if (dist < bestDist2) bestDist2 = dist;
        }
        if (bestDist <= TH_LOW_ && (float)bestDist < (float)bestDist2 * nnratio) {
            if (matches21[bestIdx2] >= 0) { matches12[matches21[bestIdx2]] = -1; nmatches--; }
            matches12[i1] = bestIdx2;
            matches21[bestIdx2] = i1;
            matchedDist[bestIdx2] = bestDist;
            nmatches++;
            if (check_orientation) {
                float rot = k1[i1].angle - k2[bestIdx2].angle;
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)roundf(rot * factor);
                if (bin == HISTO) bin = 0;
                if (bin >= 0 && bin < HISTO) rotHist[bin].push_back(i1);
            }
        }
    }
    if (check_orientation) {
        int32_t sizes[30]; int i1, i2, i3;
        for (int i = 0; i < HISTO; ++i) sizes[i] = (int)rotHist[i].size();
        orbx_three_maxima(sizes, HISTO, &i1, &i2, &i3);
        for (int i = 0; i < HISTO; ++i) {
            if (i == i1 || i == i2 || i == i3) continue;
            for (int idx1 : rotHist[i])
                if (matches12[idx1] >= 0) { matches12[idx1] = -1; nmatches--; }
        }
    }
    for (int i = 0; i < n1; ++i)
        if (matches12[i] >= 0) { prev_matched[2 * i] = k2[matches12[i]].x; prev_matched[2 * i + 1] = k2[matches12[i]].y; }
    *nmatches_out = nmatches;
    return ORBX_OK;
}
