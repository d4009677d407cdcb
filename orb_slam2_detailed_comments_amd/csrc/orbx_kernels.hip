// orbx_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the ORB front-end.
//
// Integer / byte work bound by HBM + LDS, no MFMA.  One launch handles a whole batch of frames
// (grid.y/z = frame), image tiles are staged in LDS, per-cell keypoint compaction uses wave ballot +
// mbcnt prefix, and the quadtree of one (frame, level) runs inside one workgroup with its node list in LDS.
//
// Built with -ffp-contract=off: no implicit FMA anywhere; the only fused operations are the explicit
// __builtin_fmaf calls of the descriptor taps (fp_mode GCC_FMA) and the fma() of the pinned sincos.
#include "orbx_device.h"
#include "orbx_inplace.h"
#include "orbx_fast_net.h"
#include "orbx_track.h"
#include "orbx_launch.h"   // the launch regimes (MT_SPLIT, MT_QPW, FR_GPW and the plan functions) ahead of the kernels
#include "../../include/orbx_pattern_data.h"

// ------------------------------------------------------------------------------------------------
// K0: level 0 = reflect-101 border of the input (reference src/ORBextractor.cc:2159-2163)
// one thread -> 4 horizontally adjacent padded pixels (one dword store)
// ------------------------------------------------------------------------------------------------
#define L0_ROWS 8   // rows per thread: 8 independent row loads in flight per lane (the kernel is pure streaming)
// Grid order: workgroups are dealt round-robin over the 8 XCDs (each with its own L2), so with the FRAME as the fastest grid
// dimension (batch % 8 == 0) every block of one frame lands on the same XCD and the source lines two neighbouring blocks
// both touch (strip seams, reflected rows, the border block's byte gathers) are fetched from HBM once instead of once per XCD.
// k_pyr_l0, the resize kernels and k_quadtree all take the frame from blockIdx.x for this reason.
// k_quadtree: keys a thread may keep in registers (the register path covers QT_KPT * workgroup size keys)
#define QT_KPT ORBX_QT_KPT
#ifndef QT_CENSUS_NODES
#define QT_CENSUS_NODES 1   // register path: a list of at most this many nodes (and the root bins) is counted per wave with ballots;
                            // 0 = atomics per key.  Measured at 1 (107 us), 4 (116) and 0 (136 us per 1024 frames of 640x480)
#endif
#ifndef QT_BGRP
#define QT_BGRP 3           // stage B on the register path: keys whose node reads are in flight together (divides QT_KPT)
#endif
static_assert(QT_KPT % QT_BGRP == 0, "QT_BGRP must divide QT_KPT");
#define QT_SHARED_BYTES 144
__global__ __launch_bounds__(256) void k_pyr_l0(DGeom g, const uint8_t *__restrict__ imgs, int W, int H, int stride,
                                                long long frame_stride, uint8_t *__restrict__ pyr, int xe,
                                                int *__restrict__ status, int *__restrict__ cand_cursor) {
    // block = 64 x 4 threads, thread = L0_ROWS rows.  Blocks with bx < nbx - 1 copy the interior
    // columns [32, xe) with dword-aligned loads + funnel shifts (16 pixels per thread and row); the LAST block column
    // owns the two border strips [0, 32) and [xe, pitch) where reflect-101 reverses the byte order (byte gathers).
    // Keeping the two roles in different blocks keeps every wave free of divergence.
    const DLevel &L = g.lv[0];
    const int f = blockIdx.x, bx = blockIdx.y, by = blockIdx.z, nbx = gridDim.y;
    // the per-frame status word (atomicMax'ed by the later kernels of the batch) is reset here: level 0 is the first kernel of
    // every batch, which saves a separate clearing launch in front of it
    if (bx == 0 && by == 0 && threadIdx.y == 0) {
        if (threadIdx.x == 0) status[f] = 0;
        if ((int)threadIdx.x < g.nlevels) cand_cursor[f * g.nlevels + threadIdx.x] = 0;   // appended to by k_fast_rows
    }
    const int Y0 = (by * 4 + threadIdx.y) * L0_ROWS;
    if (Y0 >= L.ph) return;
    const uint8_t *img = imgs + (long long)f * frame_stride;
    uint8_t *dst = pyr + (long long)f * g.pyr_bytes + L.off;
    if (bx + 1 < nbx) {
        const int X = 32 + (bx * 64 + threadIdx.x) * 16;
        if (X >= xe) return;
        uint4 v[L0_ROWS];
#pragma unroll
        for (int r = 0; r < L0_ROWS; ++r) {
            const int Y = min(Y0 + r, L.ph - 1);
            const uint8_t *sp = img + (long long)orbx_reflect101(Y - ORBX_EDGE, H) * stride + (X - ORBX_EDGE);
            const uint32_t m = (uint32_t)((unsigned long long)sp & 3ull);
            const uint32_t *ap = (const uint32_t *)(sp - m);
            const uint32_t q0 = ap[0], q1 = ap[1], q2 = ap[2], q3 = ap[3], q4 = ap[4];
            v[r] = make_uint4(__builtin_amdgcn_alignbyte(q1, q0, m), __builtin_amdgcn_alignbyte(q2, q1, m),
                              __builtin_amdgcn_alignbyte(q3, q2, m), __builtin_amdgcn_alignbyte(q4, q3, m));
        }
#pragma unroll
        for (int r = 0; r < L0_ROWS; ++r)
            if (Y0 + r < L.ph) *(uint4 *)(dst + (long long)(Y0 + r) * L.pitch + X) = v[r];   // pitch % 64 == 0
    } else {
        // border strips: dword e < 8 -> X = 4e (left 32 px); e >= 8 -> X = xe + 4(e - 8) (right, up to the pitch)
        const int e = threadIdx.x;
        const int X = e < 8 ? 4 * e : xe + 4 * (e - 8);
        if (X >= L.pitch) return;
#pragma unroll
        for (int r = 0; r < L0_ROWS; ++r) {
            const int Y = Y0 + r;
            if (Y >= L.ph) break;
            const uint8_t *src = img + (long long)orbx_reflect101(Y - ORBX_EDGE, H) * stride;
            uint32_t w = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int x = X + i;
                const uint32_t p = x < L.pw ? src[orbx_reflect101(x - ORBX_EDGE, W)] : 0u;
                w |= p << (8 * i);
            }
            *(uint32_t *)(dst + (long long)Y * L.pitch + X) = w;
        }
    }
}

// K0c: level 0 straight from an interleaved colour frame: cv::cvtColor(CV_RGB2GRAY / BGR / RGBA / BGRA) of
// Tracking::GrabImage* (reference src/Tracking.cc:245-271, 302-320, 372-385) fused into the border kernel.
// OpenCV 3.2 8-bit formula: gray = (R*4899 + G*9617 + B*1868 + 8192) >> 14.  thread = 4 padded pixels.
__global__ __launch_bounds__(256) void k_pyr_l0_color(DGeom g, const uint8_t *__restrict__ imgs, int W, int H, int stride,
                                                      long long frame_stride, uint8_t *__restrict__ pyr, int nch,
                                                      int r_off, int b_off, int *__restrict__ status, int *__restrict__ cand_cursor) {
    const DLevel &L = g.lv[0];
    const int X = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int Y = blockIdx.y * 4 + threadIdx.y;
    const int f = blockIdx.z;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.y == 0) {
        if (threadIdx.x == 0) status[f] = 0;
        if ((int)threadIdx.x < g.nlevels) cand_cursor[f * g.nlevels + threadIdx.x] = 0;
    }
    if (X >= L.pw || Y >= L.ph) return;
    const uint8_t *src = imgs + (long long)f * frame_stride + (long long)orbx_reflect101(Y - ORBX_EDGE, H) * stride;
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = X + i;
        uint32_t p = 0;
        if (x < L.pw) {
            const uint8_t *px = src + (long long)orbx_reflect101(x - ORBX_EDGE, W) * nch;
            p = (uint32_t)(px[r_off] * 4899 + px[1] * 9617 + px[b_off] * 1868 + 8192) >> 14;
        }
        v |= p << (8 * i);
    }
    *(uint32_t *)(pyr + (long long)f * g.pyr_bytes + L.off + (long long)Y * L.pitch + X) = v;
}

// cv::remap(INTER_LINEAR, float maps) of the EuRoC rectification (reference Examples/Stereo/stereo_euroc.cc:183-194)
// fused into the border kernel: padded pixel P of level 0 = rectified pixel at reflect101(P - 19), and a rectified pixel is
// the 5-bit fixed-point bilinear sample of the RAW image the host pre-digested map entry names (OpenCV 3.2 arithmetic:
// weights (32-fx)(32-fy)*32 ... summing to 2^15, + 2^14, >> 15; taps outside the raw image read 0).  The fx = fy = 0 entry of
// OpenCV's table is {32767, 0, 0, 1}: for 8-bit data that gives the same value as {32768, 0, 0, 0} (oracle keeps it literal).
// rect entry: .x = ix | iy << 16 (int16 each), .y = fy << 5 | fx.  thread = 4 padded pixels.
__global__ __launch_bounds__(256) void k_pyr_l0_remap(DGeom g, const uint8_t *__restrict__ imgs, int W, int H, int stride,
                                                      long long frame_stride, uint8_t *__restrict__ pyr,
                                                      const uint2 *__restrict__ rect, int *__restrict__ status,
                                                      int *__restrict__ cand_cursor) {
    const DLevel &L = g.lv[0];
    const int X = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int Y = blockIdx.y * 4 + threadIdx.y;
    const int f = blockIdx.z;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.y == 0) {
        if (threadIdx.x == 0) status[f] = 0;
        if ((int)threadIdx.x < g.nlevels) cand_cursor[f * g.nlevels + threadIdx.x] = 0;
    }
    if (X >= L.pw || Y >= L.ph) return;
    const uint8_t *src = imgs + (long long)f * frame_stride;
    const uint2 *mrow = rect + (long long)orbx_reflect101(Y - ORBX_EDGE, H) * W;
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = X + i;
        uint32_t p = 0;
        if (x < L.pw) {
            const uint2 m = mrow[orbx_reflect101(x - ORBX_EDGE, W)];
            const int ix = (int)(short)(m.x & 0xffffu), iy = (int)(short)(m.x >> 16);
            const uint32_t fx = m.y & 31u, fy = (m.y >> 5) & 31u;
            const bool x0 = ix >= 0 && ix < W, x1 = ix + 1 >= 0 && ix + 1 < W, y0 = iy >= 0 && iy < H, y1 = iy + 1 >= 0 && iy + 1 < H;
            const uint8_t *r0 = src + (long long)iy * stride + ix, *r1 = r0 + stride;
            const uint32_t p00 = (x0 && y0) ? r0[0] : 0u, p01 = (x1 && y0) ? r0[1] : 0u, p10 = (x0 && y1) ? r1[0] : 0u,
                           p11 = (x1 && y1) ? r1[1] : 0u;
            const uint32_t acc = __umul24((32u - fx) * (32u - fy) * 32u, p00) + __umul24(fx * (32u - fy) * 32u, p01) +
                                 __umul24((32u - fx) * fy * 32u, p10) + __umul24(fx * fy * 32u, p11);
            p = (acc + (1u << 14)) >> 15;
        }
        v |= p << (8 * i);
    }
    *(uint32_t *)(pyr + (long long)f * g.pyr_bytes + L.off + (long long)Y * L.pitch + X) = v;
}

// ------------------------------------------------------------------------------------------------
// K1: level l = cv::resize(INTER_LINEAR) of the PADDED level l-1 into the centre + reflect-101 border,
// in one pass: the border is produced by evaluating the bilinear formula at the reflected coordinate
// (taps precomputed per padded coordinate on the host).  (reference :2119-2143)
// ------------------------------------------------------------------------------------------------
struct __attribute__((packed, aligned(1))) orbx_uint2_u { uint32_t x, y; };   // 8 bytes at any byte address (global memory takes unaligned accesses)
struct __attribute__((packed, aligned(1))) orbx_uint3_u { uint32_t x, y, z; };
__device__ __forceinline__ uint2 orbx_load8(const void *p) { const orbx_uint2_u v = *(const orbx_uint2_u *)p; return make_uint2(v.x, v.y); }
struct __attribute__((aligned(4))) orbx_uint3_a { uint32_t x, y, z; };   // 12 bytes at a dword-aligned address
typedef unsigned short orbx_v2u16 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t orbx_udot2(uint32_t a, uint32_t b) {   // a.lo * b.lo + a.hi * b.hi, exact
    return __builtin_amdgcn_udot2(__builtin_bit_cast(orbx_v2u16, a), __builtin_bit_cast(orbx_v2u16, b), 0u, false);
}
#define RS_ROWS 2   // destination rows per thread: the horizontal taps and byte selectors are shared, 12 loads in flight
__global__ __launch_bounds__(256) void k_pyr_resize(DGeom g, int level, const OrbxTap *__restrict__ taps,
                                                    uint8_t *__restrict__ pyr) {
    // block = 64 x 4 threads; thread = 4 horizontally adjacent destination pixels x RS_ROWS rows (dword stores).
    // Products are written with __mul24 (weights <= 2048, T >> 4 <= 32640): v_mul_lo_u32 is a quarter-rate instruction.
    // The <= 8 source pixels a thread needs per source row sit inside 3 aligned dwords: 6 dword loads per
    // destination row replace 16 byte gathers (byte-gather fallback for exotic scale factors whose footprint
    // exceeds 12 bytes).
    const DLevel &L = g.lv[level];
    const DLevel &S = g.lv[level - 1];
    const int X = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int Y0 = (blockIdx.y * 4 + threadIdx.y) * RS_ROWS;
    const int f = blockIdx.z;
    if (X >= L.pw || Y0 >= L.ph) return;
    uint8_t *base = pyr + (long long)f * g.pyr_bytes;
    OrbxTap tx[4];
    int smin = 0x7fff, smax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        tx[i] = taps[L.tapx + min(X + i, L.pw - 1)];
        smin = min(smin, (int)tx[i].s0);
        smax = max(smax, (int)tx[i].s0);
    }
    OrbxTap ty[RS_ROWS];
    if (smax + 2 - smin <= 8) {
        // ---- narrow footprint (every usual scale factor): the <= 8 source bytes a thread needs per source row come
        // with ONE unaligned 8-byte load; v_perm_b32 puts the two taps of a destination pixel into the 16-bit halves
        // of a register and v_dot2_u32_u16 against the packed weights (a0 | a1 << 16 = the second dword of the tap
        // record) is the horizontal pass: two instructions per pixel and source row, no selects, no multiplies.
        uint32_t sel[4], wgt[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t d = (uint32_t)(tx[i].s0 - smin);              // 0..6; second tap = next byte (weight 0 when clamped)
            sel[i] = d | (0x0cu << 8) | ((d + 1u) << 16) | (0x0cu << 24);   // 0x0c selects the constant 0x00
            wgt[i] = (uint32_t)(uint16_t)tx[i].a0 | ((uint32_t)(uint16_t)tx[i].a1 << 16);
        }
        uint2 u[RS_ROWS], w[RS_ROWS];
#pragma unroll
        for (int r = 0; r < RS_ROWS; ++r) {
            ty[r] = taps[L.tapy + min(Y0 + r, L.ph - 1)];
            u[r] = orbx_load8(base + S.off + (long long)ty[r].s0 * S.pitch + smin);
            w[r] = orbx_load8(base + S.off + (long long)ty[r].s1 * S.pitch + smin);
        }
#pragma unroll
        for (int r = 0; r < RS_ROWS; ++r) {
            const int Y = Y0 + r;
            if (Y >= L.ph) break;
            const uint32_t b0 = (uint32_t)ty[r].a0 & 0xfffu, b1 = (uint32_t)ty[r].a1 & 0xfffu;
            uint32_t v = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t T0 = orbx_udot2(__builtin_amdgcn_perm(u[r].y, u[r].x, sel[i]), wgt[i]);
                const uint32_t T1 = orbx_udot2(__builtin_amdgcn_perm(w[r].y, w[r].x, sel[i]), wgt[i]);
                const uint32_t p = ((__umul24(b0, T0 >> 4) >> 16) + (__umul24(b1, T1 >> 4) >> 16) + 2u) >> 2;   // <= 255
                v |= p << (8 * i);
            }
            *(uint32_t *)(base + L.off + (long long)Y * L.pitch + X) = v;
        }
        return;
    }
    const int xb = smin & ~3;
    const bool windowed = smax + 1 - xb < 12;
    uint32_t u[RS_ROWS][3], w[RS_ROWS][3];
#pragma unroll
    for (int r = 0; r < RS_ROWS; ++r) {
        ty[r] = taps[L.tapy + min(Y0 + r, L.ph - 1)];
        if (windowed) {
            const uint32_t *q0 = (const uint32_t *)(base + S.off + (long long)ty[r].s0 * S.pitch + xb);
            const uint32_t *q1 = (const uint32_t *)(base + S.off + (long long)ty[r].s1 * S.pitch + xb);
            u[r][0] = q0[0]; u[r][1] = q0[1]; u[r][2] = q0[2];
            w[r][0] = q1[0]; w[r][1] = q1[1]; w[r][2] = q1[2];
        }
    }
#pragma unroll
    for (int r = 0; r < RS_ROWS; ++r) {
        const int Y = Y0 + r;
        if (Y >= L.ph) break;
        const int b0 = ty[r].a0, b1 = ty[r].a1;
        uint32_t v = 0;
        if (windowed) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idx = tx[i].s0 - xb;  // 0..10; the second tap is the next byte (weight 0 whenever clamped)
                const uint32_t ulo = idx < 4 ? u[r][0] : idx < 8 ? u[r][1] : u[r][2], uhi = idx < 4 ? u[r][1] : idx < 8 ? u[r][2] : 0u;
                const uint32_t wlo = idx < 4 ? w[r][0] : idx < 8 ? w[r][1] : w[r][2], whi = idx < 4 ? w[r][1] : idx < 8 ? w[r][2] : 0u;
                const uint32_t pu = __builtin_amdgcn_alignbyte(uhi, ulo, (uint32_t)idx & 3u);
                const uint32_t pw_ = __builtin_amdgcn_alignbyte(whi, wlo, (uint32_t)idx & 3u);
                const int T0 = (int)(pu & 0xff) * tx[i].a0 + (int)((pu >> 8) & 0xff) * tx[i].a1;
                const int T1 = (int)(pw_ & 0xff) * tx[i].a0 + (int)((pw_ >> 8) & 0xff) * tx[i].a1;
                const uint32_t p = (uint32_t)((((((b0 & 0xfff) * ((T0 >> 4) & 0xffff))) >> 16) + ((((b1 & 0xfff) * ((T1 >> 4) & 0xffff))) >> 16) + 2) >> 2) & 0xffu;
                v |= p << (8 * i);
            }
        } else {
            const uint8_t *r0 = base + S.off + (long long)ty[r].s0 * S.pitch;
            const uint8_t *r1 = base + S.off + (long long)ty[r].s1 * S.pitch;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int T0 = r0[tx[i].s0] * tx[i].a0 + r0[tx[i].s1] * tx[i].a1;
                const int T1 = r1[tx[i].s0] * tx[i].a0 + r1[tx[i].s1] * tx[i].a1;
                const uint32_t p = (uint32_t)((((((b0 & 0xfff) * ((T0 >> 4) & 0xffff))) >> 16) + ((((b1 & 0xfff) * ((T1 >> 4) & 0xffff))) >> 16) + 2) >> 2) & 0xffu;
                v |= p << (8 * i);
            }
        }
        *(uint32_t *)(base + L.off + (long long)Y * L.pitch + X) = v;
    }
}

// Row-walking form of the narrow-footprint path (the one every usual geometry takes; the host checks the tap table and
// launches k_pyr_resize above otherwise).  k_pyr_resize is latency-bound: tap records -> source loads -> store is a
// chain of two dependent global loads per 512 bytes written.  Here a wave keeps its column strip's horizontal selectors /
// weights in registers and walks `rpw` destination rows: the vertical taps are scalar loads (the row is wave-uniform),
// the source rows of step k+1 are requested before step k is evaluated, and nothing in the loop waits on a table.
// (A variant that lays (row pair, dword) items out linearly over the lanes to remove the idle lanes of odd level widths
// measured 258 us against 207 us: vector tap loads, rows split across a wave.)
#ifndef RR_WPB
#define RR_WPB 1   // waves (column strips x row ranges) per block; nothing is shared between them, and one-wave blocks
                   // are placed as soon as any SIMD has room (201 us against 209 with 4)
#endif
// ---- The row walk itself, shared by k_pyr_resize_rows and k_pyr_resize_rows_l1 (which differ in how a source row is loaded
// and in how the byte selectors are built).
// the vertical tap records of two consecutive destination rows, at any dword address: (.x, .y) = row Y, (.z, .w) = row Y + 1,
// each s0 | s1 << 16, a0 | a1 << 16
typedef uint32_t orbx_tap2 __attribute__((ext_vector_type(4), aligned(4)));
// The tap table is written by the host before any launch and never by a kernel: a pointer into it in the constant address
// space makes every fetch of a pair a scalar load (as a global pointer the fetches behind the loop's first store became
// vector loads + v_readfirstlane, and a wait for every load in flight)
typedef const __attribute__((address_space(4))) orbx_tap2 *rr_tap2_ptr;
__device__ __forceinline__ rr_tap2_ptr rr_tap_pairs(const OrbxTap *p) { return (rr_tap2_ptr)(uintptr_t)p; }
struct RrLoad12 {   // slab rows, and body strips of the caller's image: the dword-aligned 12-byte window from column `col`
    const uint8_t *src;
    uint32_t pitch, col;
    __device__ __forceinline__ orbx_uint3_a operator()(uint32_t row) const {
        return *(const orbx_uint3_a *)(src + orbx_ip_row_off((int)row, (int)pitch, (int)col));
    }
};
struct RrLoad8 {    // tail strips of the caller's image: 8 bytes at byte alignment from column `col`
    const uint8_t *src;
    uint32_t pitch, col;
    __device__ __forceinline__ orbx_uint3_a operator()(uint32_t row) const {
        const uint2 q = orbx_load8(src + orbx_ip_row_off((int)row, (int)pitch, (int)col));
        orbx_uint3_a v;
        v.x = q.x; v.y = q.y; v.z = 0;
        return v;
    }
};
__device__ __forceinline__ uint32_t orbx_mulhi24(uint32_t a, uint32_t b) {   // (a * b) >> 32 of two 24-bit values: v_mul_hi_u32_u24, full rate
    return (uint32_t)(((uint64_t)(a & 0xffffffu) * (uint64_t)(b & 0xffffffu)) >> 32);
}
__device__ __forceinline__ uint32_t rr_pin(uint32_t v) {   // a wave-uniform loop constant: held in its scalar register, not re-read
    asm volatile("" : "+s"(v));                            // from the kernel arguments inside the loop
    return v;
}
// The lane's four horizontal tap records, addressed as the table's scalar base + a 32-bit offset
__device__ __forceinline__ void rr_taps_x(const OrbxTap *__restrict__ tq, int X, int pw, uint2 (&t)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = *(const uint2 *)((const uint8_t *)tq + (uint32_t)min(X + i, pw - 1) * 8u);   // .x = s0 | s1 << 16, .y = a0 | a1 << 16
}
// Destination rows [Y, Y + n) of a column strip, n >= 1; tp = the vertical tap record of row Y (the table carries one record
// beyond its level's last row, so the second record of the pair a range ends on may be read whatever n is); vdst = byte offset
// of the lane's dword in row Y, dpitch = bytes between destination rows.
//
// Two destination rows per step.  The horizontal pass of a SOURCE row (h[i] = (a0 * p[s0] + a1 * p[s0+1]) >> 4 for the
// lane's four columns; held as h << 4) is what cv::resize keeps in its row buffers: destination row Y+1 usually starts on the source row
// destination row Y ended on (scale 1.2: 2.4 new source rows per two destination rows instead of 4), so the last row's
// h values stay in registers (source row `pid`; hb[0] / hb[1] alternate as "row s0" / "row s1", nothing is copied) and only
// rows not seen yet are loaded and filtered -- 40 % fewer loads, 22 % fewer vector instructions per pixel.  All conditions
// are wave-uniform (scalar branches).
// The rows of step k+1 are requested before step k is evaluated.  The two register sets this needs (A, B: tap records + up to
// four source rows each) swap roles by code position -- a trip of the loop is two steps, A then B -- not by moving values.
template <class LD>
__device__ __forceinline__ void rr_walk(const LD ld, const uint32_t (&sel)[4], const uint32_t (&wgt)[4], const uint32_t sh,
                                        rr_tap2_ptr tp, uint8_t *__restrict__ dst, uint32_t vdst,
                                        const uint32_t dpitch, int n) {
    // the four pixels are taken through each stage together: no v_dot2 result is shifted by the instruction behind it
#define RR_H(h, v)                                                                                                       \
    {                                                                                                                   \
        const uint32_t lo_ = __builtin_amdgcn_alignbyte((v).y, (v).x, sh), hi_ = __builtin_amdgcn_alignbyte((v).z, (v).y, sh); \
        uint32_t p_[4];                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) p_[i] = __builtin_amdgcn_perm(hi_, lo_, sel[i]);                  \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) p_[i] = orbx_udot2(p_[i], wgt[i]);                                \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) h[i] = p_[i] & 0xfffff0u;   /* ((a0 p0 + a1 p1) >> 4) << 4 */     \
    }
    // Vertical pass, the integers of cv::resize: ((b0 * T0 >> 16) + (b1 * T1 >> 16) + 2) >> 2 with T = the horizontal value >> 4.
    // The h values are kept as T << 4 (one v_and instead of one shift) and the 12-bit weights as b << 12, so that the high half of
    // the 24 x 24-bit product (v_mul_hi_u32_u24) IS b * T >> 16: two multiplies and one add per pixel.  The four
    // sums (<= 1020) are packed in pairs, get their + 2 together and are shifted by 6: byte 1 / byte 3 of a pair are its two pixels,
    // one v_perm gathers them.
#define RR_V(out, h0, h1, ty_)                                                                                          \
    {                                                                                                                   \
        const uint32_t w0_ = ((ty_) << 12) & 0xfff000u, w1_ = ((ty_) >> 4) & 0xfff000u;                                 \
        uint32_t s_[4];                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) s_[i] = orbx_mulhi24(w0_, h0[i]) + orbx_mulhi24(w1_, h1[i]);      \
        out = __builtin_amdgcn_perm((((s_[3] << 16) + s_[2]) + 0x00020002u) << 6, (((s_[1] << 16) + s_[0]) + 0x00020002u) << 6, \
                                    0x07050301u);                                                                      \
    }
    // a set's rows, skipping the rows the step before it leaves filtered in registers (`last`: that step's final source row)
#define RR_FETCH(S, last)                                                                                               \
    {                                                                                                                   \
        S##t = *tp++;                                                                                                   \
        if ((S##t.x & 0xffffu) != (uint32_t)(last)) S##u0 = ld(S##t.x & 0xffffu);                                     \
        S##w0 = ld(S##t.x >> 16);                                                                                      \
        if ((S##t.z & 0xffffu) != (S##t.x >> 16)) S##u1 = ld(S##t.z & 0xffffu);                                      \
        S##w1 = ld(S##t.z >> 16);                                                                                      \
    }
    // the set's two destination rows (the second one stored only if the range has it: rows > 1)
#define RR_EVAL(S, rows)                                                                                                \
    {                                                                                                                   \
        uint32_t v_;                                                                                                    \
        if ((S##t.x & 0xffffu) != pid) RR_H(hb[0], S##u0)                                                              \
        RR_H(hb[1], S##w0)                                                                                              \
        RR_V(v_, hb[0], hb[1], S##t.y)                                                                                 \
        *(uint32_t *)(dst + vdst) = v_;                                                                                 \
        vdst += dpitch;                                                                                                 \
        if ((S##t.z & 0xffffu) != (S##t.x >> 16)) RR_H(hb[1], S##u1)                                                  \
        RR_H(hb[0], S##w1)                                                                                              \
        RR_V(v_, hb[1], hb[0], S##t.w)                                                                                 \
        if ((rows) > 1) *(uint32_t *)(dst + vdst) = v_;                                                                 \
        vdst += dpitch;                                                                                                 \
        pid = S##t.z >> 16;                                                                                            \
    }
    orbx_tap2 At, Bt;
    orbx_uint3_a Au0, Aw0, Au1, Aw1, Bu0, Bw0, Bu1, Bw1;
    Au0.x = Au0.y = Au0.z = 0;   // a row that is not loaded is not read either; the zeros only give the registers a defined value
    Au1 = Bu0 = Bu1 = Au0;
    uint32_t pid = 0xffffffffu;                     // source row whose horizontal pass hb[0] holds at the top of a step
    uint32_t hb[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    RR_FETCH(A, 0xffffffffu)
    for (;;) {
        if (n > 2) RR_FETCH(B, At.z >> 16)
        RR_EVAL(A, n)
        if (n <= 2) break;
        if (n > 4) RR_FETCH(A, Bt.z >> 16)
        RR_EVAL(B, n - 2)
        if (n <= 4) break;
        n -= 4;
    }
#undef RR_H
#undef RR_V
#undef RR_FETCH
#undef RR_EVAL
}
__global__ __launch_bounds__(64 * RR_WPB) void k_pyr_resize_rows(DGeom g, int level, const OrbxTap *__restrict__ taps,
                                                         uint8_t *__restrict__ pyr, int rpw) {
    const DLevel &L = g.lv[level];
    const DLevel &S = g.lv[level - 1];
    const int lane = threadIdx.x;
    // Odd levels walk their row ranges bottom-up: with the frame as the fastest grid index the launch that wrote level l-1
    // finished with the bottom rows of every frame, and what the memory-side cache still holds of that level is those rows
    const int f = blockIdx.x, bx = blockIdx.y;
    const int by = (level & 1) ? (int)gridDim.z - 1 - (int)blockIdx.z : (int)blockIdx.z;
    const int X = (bx * 64 + lane) * 4;
    const int y_begin = __builtin_amdgcn_readfirstlane((by * RR_WPB + threadIdx.y) * rpw);
    if (y_begin >= L.ph) return;
    const int y_end = min(y_begin + rpw, L.ph);
    if (X >= L.pw) return;   // lanes beyond the level's width (the last strip) are done: no load, no store, no mask around the stores
    uint8_t *base = pyr + (long long)f * g.pyr_bytes;
    const uint8_t *src = base + S.off;
    // Addresses = the level's wave-uniform base (the scalar operand of the loads and stores, saddr form) + a 32-bit offset
    // (scalar row * pitch + the lane's column: one v_add per access; a level is far below 4 GB) -- round 2's form paid a 64-bit
    // vector multiply-add per row load (v_mad_i64_i32) and per store (v_mad_u64_u32)
    uint8_t *dst = base + L.off;
    const uint32_t spitch = rr_pin((uint32_t)S.pitch), dpitch = rr_pin((uint32_t)L.pitch);
    uint32_t sel[4], wgt[4];
    int smin = 0x7fff;
    {
        uint2 t[4];
        rr_taps_x(taps + L.tapx, X, L.pw, t);
#pragma unroll
        for (int i = 0; i < 4; ++i) smin = min(smin, (int)(t[i].x & 0xffffu));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t d = (t[i].x & 0xffffu) - (uint32_t)smin;          // 0..6 (checked on the host)
            sel[i] = d | (0x0cu << 8) | ((d + 1u) << 16) | (0x0cu << 24);    // the second tap is the next byte; 0x0c selects the constant 0x00
            wgt[i] = t[i].y;
        }
    }
    // A lane's 8 source bytes start at byte smin of the row: read as the dword-ALIGNED 12-byte window around them and
    // funnel-shifted in registers (two v_alignbyte).  The per-lane unaligned 8-byte load this replaces (a 4.8-byte lane
    // stride, 1-byte alignment) was what bounded the kernel: the address unit serves such a wave-load lane by lane.
    const RrLoad12 ld = {src, spitch, (uint32_t)(smin & ~3)};
    rr_walk(ld, sel, wgt, (uint32_t)(smin & 3), rr_tap_pairs(taps + L.tapy + y_begin), dst,
            (uint32_t)y_begin * dpitch + (uint32_t)X, dpitch, y_end - y_begin);
}

// Level 1 straight from the caller's grey image (in-place mode: no padded level-0 copy exists).  Same row walk, with
//   * a tap table of its own (orbx_geometry.cpp): source indices in RAW coordinates, the reflection of level 0's border folded
//     in, so the second tap of a column is no longer "the next byte": the byte selectors are built from both indices;
//   * body strips reading the dword-aligned 12-byte window, tail strips (blockIdx.y >= tail_bx, wave-uniform: the strips with
//     a lane whose window would leave its source row) reading 8 bytes at byte alignment from min(lo, W - 8);
//   * the two side duties of k_pyr_l0 (it is the first launch of a batch on its stream now): status[f] and cand_cursor[f][*].
// Address arithmetic: orbx_inplace.h.
template <bool TAIL>
__device__ __forceinline__ void rr_l1_body(const DLevel &L, const OrbxTap *__restrict__ taps, const uint8_t *__restrict__ src,
                                           int W, int stride, uint8_t *__restrict__ dst, int X, int y_begin, int y_end) {
    const uint32_t spitch = rr_pin((uint32_t)stride), dpitch = rr_pin((uint32_t)L.pitch);
    uint32_t sel[4], wgt[4];
    int lo = 0x7fff;
    {
        uint2 t[4];
        rr_taps_x(taps, X, L.pw, t);
#pragma unroll
        for (int i = 0; i < 4; ++i) lo = min(lo, (int)min(t[i].x & 0xffffu, t[i].x >> 16));
        const int org = TAIL ? orbx_ip_rr_tail_col(lo, W) : lo;       // raw column of byte 0 of the lane's 8-byte register pair
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t d0 = (t[i].x & 0xffffu) - (uint32_t)org, d1 = (t[i].x >> 16) - (uint32_t)org;   // 0..7 (checked on the host)
            sel[i] = d0 | (0x0cu << 8) | (d1 << 16) | (0x0cu << 24);
            wgt[i] = t[i].y;
        }
    }
    const rr_tap2_ptr tp = rr_tap_pairs(taps + L.pw + y_begin);
    const uint32_t vdst = (uint32_t)y_begin * dpitch + (uint32_t)X;
    if (TAIL) {
        const RrLoad8 ld = {src, spitch, (uint32_t)orbx_ip_rr_tail_col(lo, W)};
        rr_walk(ld, sel, wgt, 0u, tp, dst, vdst, dpitch, y_end - y_begin);
    } else {
        const RrLoad12 ld = {src, spitch, (uint32_t)orbx_ip_rr_body_col(lo)};
        rr_walk(ld, sel, wgt, (uint32_t)(lo & 3), tp, dst, vdst, dpitch, y_end - y_begin);
    }
}
__global__ __launch_bounds__(64 * RR_WPB) void k_pyr_resize_rows_l1(DGeom g, const OrbxTap *__restrict__ taps, OrbxRaw0 raw,
                                                            uint8_t *__restrict__ pyr, int rpw, int tail_bx,
                                                            int *__restrict__ status, int *__restrict__ cand_cursor) {
    const DLevel &L = g.lv[1];
    const int lane = threadIdx.x;
    const int f = blockIdx.x, bx = blockIdx.y;
    const int by = (int)gridDim.z - 1 - (int)blockIdx.z;   // level 1 is odd: bottom-up, as in k_pyr_resize_rows
    const bool first = blockIdx.y == 0 && blockIdx.z == 0;
    if (first && threadIdx.y == 0 && status) {   // one block per frame, as k_pyr_l0 does in the eager mode; null: the caller has reset them
        if (lane == 0) status[f] = 0;
        if (lane < g.nlevels) cand_cursor[f * g.nlevels + lane] = 0;
    }
    const int X = (bx * 64 + lane) * 4;
    const int y_begin = __builtin_amdgcn_readfirstlane((by * RR_WPB + threadIdx.y) * rpw);
    if (y_begin >= L.ph) return;
    const int y_end = min(y_begin + rpw, L.ph);
    if (X >= L.pw) return;   // as k_pyr_resize_rows
    const uint8_t *src = raw.img + (long long)f * raw.frame_stride;
    uint8_t *dst = pyr + (long long)f * g.pyr_bytes + L.off;
    if (bx >= tail_bx) rr_l1_body<true>(L, taps, src, raw.W, raw.stride, dst, X, y_begin, y_end);
    else rr_l1_body<false>(L, taps, src, raw.W, raw.stride, dst, X, y_begin, y_end);
}

// ------------------------------------------------------------------------------------------------
// K2: FAST-9/16 + score + 3x3 strict NMS per cell, with the per-cell threshold retry
// (reference src/ORBextractor.cc:1465-1548; cv::FAST semantics SURVEY App. B.1): helpers, then k_fast_rows.
// ------------------------------------------------------------------------------------------------
// dynamic LDS: tile[rows*TP] | score[rows*TP] | list u16[lcap] (two-ended) | corn u16[lcap]; TP = tile pitch (%4 == 0)
// ballot straight from the compare's lane mask (HIP's __ballot goes through an int and costs v_cndmask + v_cmp)
__device__ __forceinline__ unsigned long long orbx_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int orbx_wave_rank(unsigned long long bal) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
}
// LDS traffic inside one wave is ordered by the hardware; this only stops the compiler from reordering across phases
__device__ __forceinline__ void orbx_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------------------
// k_fast_rows: per-cell FAST-9/16 + score + NMS + threshold retry, organised so that the dense part costs a dozen vector
// instructions per image ROW (the first version, one wave per cell with a compass test per pixel pair, took 532 us per
// 256 frames against 390 us; git history has it):
//   * one wave owns a GROUP of one or two horizontally adjacent cells (OrbxFastGroup); lane i is interior column i of
//     the group and walks down the rows with the column's 7-row window in registers (one LDS byte per row), the two
//     horizontal compass pixels come from LDS with immediate offsets -- no per-pixel address arithmetic;
//   * the compass pre-test runs for ONE threshold (iniThFAST); the 4.6 % of cells that come out empty repeat the walk
//     with minThFAST (reference :1519-1527), instead of every pixel paying for both thresholds;
//   * 16-bit min/max (full rate on gfx950; the 32-bit forms are not) and a per-row ballot compaction into a bounded
//     LDS list; the list is flushed through the full ring test + score whenever the next row might not fit, so the
//     LDS footprint is independent of how many pixels pass;
//   * NMS walks the corner list when every corner of the group fitted it, otherwise it rescans the score map.
// ------------------------------------------------------------------------------------------------
#ifndef FR_TP
#define FR_TP 76        // LDS tile pitch: 64 interior columns + 6 ring + 3 alignment bytes -> 19 dwords (odd: rows spread over all banks)
#endif
// (Staging the tile by LDS-DMA -- global_load_lds_dwordx4 at pitch 80, no VGPR round trip, no ds_write pass -- was built and
// measured in round 2: bit-exact, but 408-414 us against 402 us for the register-prefetch staging below, also with the next
// tile requested before the NMS of the current one: the staging instructions are ~5 % of the kernel's issue slots and the
// register prefetch hides the load latency better than a wait on vmcnt does.  Not kept; git history has it.)
#ifndef FR_WPS
#define FR_WPS 5
#endif
#ifndef FR_CCAP
#define FR_CCAP 512     // corner-list entries per group (see orbx_launch_fast_rows, which has the byte arithmetic)
#endif
#define FR_STACK 128    // re-run stack of fr_round, entries: between the work list and the corner list
// (FR_GPW, the groups per wave of a large launch: orbx_launch.h)
typedef unsigned short fr_u16;
typedef short fr_i16;
typedef __attribute__((address_space(3))) uint16_t fr_lds_u16;
__device__ __forceinline__ fr_u16 fr_max(fr_u16 a, fr_u16 b) { return a > b ? a : b; }
__device__ __forceinline__ fr_u16 fr_min(fr_u16 a, fr_u16 b) { return a < b ? a : b; }
__device__ __forceinline__ fr_i16 fr_smax(fr_i16 a, fr_i16 b) { return a > b ? a : b; }

static_assert(64 + ORBX_FAST_XCOLS + 6 + 3 <= FR_TP, "a cell pair's tile row must fit the LDS tile pitch");
// The LDS of one wave, ONE definition for the kernel's pointers and the launcher's byte count:
//   tile | score map (each map_bytes, 16-byte aligned: cleared with 16-byte stores) | work list u16[lcap] | stack u16[FR_STACK] |
//   corner list of the group u16[ccap]
struct FrLds { int map_bytes, list_off, corn_off, bytes; };
__host__ __device__ __forceinline__ FrLds fr_lds(int rows, int lcap, int ccap) {
    FrLds l;
    l.map_bytes = (rows * FR_TP + 15) & ~15;
    l.list_off = 2 * l.map_bytes;
    l.corn_off = l.list_off + 2 * (lcap + FR_STACK);
    l.bytes = l.corn_off + 2 * ccap;
    return l;
}
static_assert(FR_STACK >= 64 + 64, "a round pushes at most 64 entries on a stack that holds at most 64 before it");
__device__ __forceinline__ bool colx_on_mask(unsigned act) { return (act & 2u) != 0; }   // columns >= 64 belong to the second cell
struct FrCtx {
    const uint8_t *tile;   // LDS tile, byte (0,0) = sub-mat origin of the group's first cell
    uint8_t *score;        // LDS score map, same coordinates
    uint16_t *list;        // LDS candidate / corner work list (lcap entries)
    uint16_t *corn;        // LDS corner list of the whole group (lcap entries)
    int lcap;
    int lane;
};

// Corner test and score of list[0..n) at threshold th in ONE pass per candidate; corners compacted IN PLACE to the front of the
// list, their scores written to the score map; returns the number of corners.
//   cv::FAST's test (9 contiguous ring pixels all brighter than v + th, or all darker than v - th) is "the largest over the 16
// arcs of the smallest signed difference on the arc exceeds th" -- which is cv::cornerScore's own quantity (score + 1).  So the
// min/max network of the score IS the test: 16-bit min / max issue at the full rate, where the ring masks of a separate test
// (v_cmp + v_addc per ring pixel and polarity) are all half-rate, and the second pass over the corners (17 LDS reads per corner
// again) disappears.  (The two-pass form with ring masks measured slower, profiles/r03_fast_onepass.md; the parent of this commit
// has the code.)
//   One polarity per candidate: the compass pixels (ring 0 / 4 / 8 / 12: the walk's pre-test) say which margin is the larger one,
// and the network runs on the raw ring bytes, complemented for the darker polarity (one xor per ring pixel), in the prefix / suffix
// form: 57 two-input operations, the centre subtracted once at the end (orbx_fast_net.h).  Two-input forms only: v_min3_i16 /
// v_max3_i16 issue at a QUARTER of the rate of v_min_i16 on gfx950 (8.4 against 2.8 cycles per wave, tools/valu_rate6.hip).
// (A doubling network on d = +-(ring - v), 80 operations behind 16 multiply-adds, measured slower, profiles/fast_net.md; the
// parent of this commit has the code.)
//   A candidate that passes BOTH pre-tests (a pixel half way
// up a strong edge: < 1 % of the candidates) and fails its larger polarity may still be a corner of the other one: it is pushed on
// a small stack (FR_STACK entries behind the work list) and re-run with the polarity
// forced the other way in a later round; the stack is drained whenever it could not take another round's worth.
// one round of up to 64 candidates.  FULL: 64 entries of the main list, every lane busy, nothing selected per lane.  Otherwise lanes
// [0, cm) take main entries and lanes [cm, cm + cs) entries popped from the stack, which run with the polarity forced the other way.
template <bool FULL>
__device__ __forceinline__ void fr_round(const FrCtx &c, const uint16_t *src_main, int cm, const uint16_t *src_stack, int cs,
                                         int th, uint16_t *stack, int &ncorn, int &nredo) {
    // offsets from the TOP-LEFT corner of the pixel's 7x7 window: none is negative, so every ring read is base + immediate (a DS
    // offset is unsigned: the seven negative offsets of a centre-based table cost a v_add each, per round)
    const int rc = 3 * FR_TP + 3;
    const int ro[16] = {rc + 3 * FR_TP,      rc + 3 * FR_TP + 1,  rc + 2 * FR_TP + 2,  rc + FR_TP + 3, rc + 3,  rc - FR_TP + 3,
                        rc - 2 * FR_TP + 2, rc - 3 * FR_TP + 1, rc - 3 * FR_TP,     rc - 3 * FR_TP - 1, rc - 2 * FR_TP - 2,
                        rc - FR_TP - 3,     rc - 3,             rc + FR_TP - 3,      rc + 2 * FR_TP - 2,  rc + 3 * FR_TP - 1};
    const bool is_main = FULL || c.lane < cm;
    uint16_t code;
    fr_i16 thl;
    if (FULL) {
        code = src_main[c.lane];
        thl = (fr_i16)th;
    } else {
        const bool valid = c.lane < cm + cs;
        const uint16_t *src = is_main ? src_main + c.lane : src_stack + (c.lane - cm);
        code = valid ? *src : (uint16_t)(3 << 8);
        // lanes without an entry carry a threshold no 8-bit difference reaches: no lane mask in the tests below
        thl = valid ? (fr_i16)th : (fr_i16)0x4000;
    }
    const int off = ((code >> 8) - 3) * FR_TP + (code & 0xff);   // window corner: row - 3, column - 3 (rows start at 3)
    const uint8_t *ptr = c.tile + off;
    // the network on the raw ring bytes, prefix / suffix form (orbx_fast_net.h); an entry from the stack takes the other polarity
    const fr_u16 v = ptr[rc];
    fr_u16 x[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = ptr[ro[k]];
    bool corner, both;
    uint8_t sc;
    orbx_fast_net(v, x, thl, !FULL && !is_main, corner, sc, both);
    const unsigned long long m = orbx_ballot(corner);
    if (corner) {
        c.list[ncorn + orbx_wave_rank(m)] = code;   // index < the entries already read: this round's are in registers
        c.score[off + rc] = sc;
    }
    ncorn += __popcll(m);
    // (the mask of the re-runs from the two compare masks on the scalar unit; per-lane work only inside the rare branch)
    unsigned long long mr = orbx_ballot(both) & ~m;
    if (!FULL) mr &= cm >= 64 ? ~0ull : ((1ull << cm) - 1ull);
    if (mr != 0ull) {
        const bool redo = both && !corner && is_main;
        if (redo) stack[nredo + orbx_wave_rank(mr)] = code;
        nredo += __popcll(mr);
    }
}
__device__ __forceinline__ int fr_ring_and_score(const FrCtx &c, int n, int th) {
    uint16_t *const stack = c.list + c.lcap;   // FR_STACK entries
    int ncorn = 0, nredo = 0, e0 = 0;
    // full rounds of the main list (a round pushes at most 64 entries: with at most 64 on the stack before it, 128 hold them)
    for (; n - e0 >= 64 && nredo <= 64; e0 += 64) fr_round<true>(c, c.list + e0, 64, stack, 0, th, stack, ncorn, nredo);
    // the rest of the main list and the stack, the stack in whatever lanes the main entries leave free
    for (;;) {
        const int cm = nredo > 64 ? 0 : min(n - e0, 64);
        const int cs = min(nredo, 64 - cm);
        if (cm + cs == 0) break;
        nredo -= cs;
        fr_round<false>(c, c.list + e0, cm, stack + nredo, cs, th, stack, ncorn, nredo);
        e0 += cm;
    }
    orbx_wave_sync();
    return ncorn;
}

// strict 3x3 NMS of list[0..n) among the corners of the SAME cell, survivors straight to the cell's slot range
struct FrCells {
    int iw0;                        // interior columns of the first cell (64 when the group is a single cell)
    int offx0, offx1, offy;         // j*wCell of the two cells, i*hCell
    int ord0, ord1;                 // idx_in_level
    int cap0, cap1;                 // slot_cap: survivors a cell may report (exact NMS worst case unless max_cand_per_cell cut it)
    uint2 *out;                     // dense candidate array of this (frame, level)
    int *cursor;                    // its fill count: one returning atomicAdd per NMS round reserves the round's survivors
    int out_cap;                    // entries the array holds
};
__device__ __forceinline__ void fr_nms(const FrCtx &c, const FrCells &gc, const uint16_t *list, int n, int &ns0, int &ns1) {
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + c.lane;
        const bool valid = e < n;
        const uint16_t code = valid ? list[e] : (uint16_t)(3 << 8);
        const int col = code & 0xff, ly = (code >> 8) & 0x7f;
        const bool second = col >= gc.iw0;
        const uint8_t *sp = c.score + (ly - 1) * FR_TP + 2 + col;   // top-left of the 3x3 neighbourhood: immediates only
        const int sc = sp[FR_TP + 1];
        const int l0 = sp[0], l1 = sp[FR_TP], l2 = sp[2 * FR_TP];
        const int r0 = sp[2], r1 = sp[FR_TP + 2], r2 = sp[2 * FR_TP + 2];
        const int u = sp[1], dn = sp[2 * FR_TP + 1];
        // the score map is shared by the two cells: the neighbours across the seam belong to the other cell's cv::FAST call
        // (strictly greater than all eight <=> strictly greater than their maximum: one select per side, not one per neighbour)
        const bool seam_l = col == gc.iw0, seam_r = col == gc.iw0 - 1;
        // (each side's maximum as ONE 32-bit three-input operation, written as the instruction: the scores are bytes, so from
        // max(max(l0, l1), l2) the compiler makes the quarter-rate v_max3_u16, and an empty asm between the two costs an s_nop)
        int ml3, mr3;
        asm("v_max3_u32 %0, %1, %2, %3" : "=v"(ml3) : "v"(l0), "v"(l1), "v"(l2));
        asm("v_max3_u32 %0, %1, %2, %3" : "=v"(mr3) : "v"(r0), "v"(r1), "v"(r2));
        const int ml = seam_l ? 0 : ml3, mr = seam_r ? 0 : mr3;
        const bool keep = (int)valid & (int)(sc > max(max(ml, mr), max(u, dn)));
        const unsigned long long m = orbx_ballot(keep), msec = orbx_ballot(keep && second);
        const unsigned long long mfirst = m & ~msec;
        const int slot = second ? ns1 + orbx_wave_rank(msec) : ns0 + orbx_wave_rank(mfirst);   // ordinal inside the cell
        const bool ok = keep && slot < (second ? gc.cap1 : gc.cap0);
        const unsigned long long mok = orbx_ballot(ok);
        if (mok != 0ull) {
            // The survivors go straight into the level's dense key array (any order: every record carries its emission-order
            // key, and the quadtree is order-free): no per-cell slot ranges, no gather pass in front of the quadtree.
            int base = 0;
            if (c.lane == 0) base = atomicAdd(gc.cursor, (int)__popcll(mok));
            base = __builtin_amdgcn_readfirstlane(base);
            const int pos = base + orbx_wave_rank(mok);
            if (ok && pos < gc.out_cap) {
                const int lx = 3 + col - (second ? gc.iw0 : 0);
                uint2 o;
                o.x = (uint32_t)(lx + (second ? gc.offx1 : gc.offx0)) | ((uint32_t)(ly + gc.offy) << 12) | ((uint32_t)sc << 24);
                o.y = ((uint32_t)(second ? gc.ord1 : gc.ord0) << 12) | ((uint32_t)ly << 6) | (uint32_t)lx;   // emission order key
                gc.out[pos] = o;
            }
        }
        ns0 += __popcll(mfirst);
        ns1 += __popcll(msec);
    }
}

// a 12-byte piece shifted right by s bytes (zeros shifted in; s >= 12 leaves nothing): the in-place pieces that were loaded
// from W - 12 because they would have left their source row (orbx_ip_fast_piece_col)
__device__ __forceinline__ orbx_uint3_u orbx_shr96(orbx_uint3_u v, int s) {
    uint32_t a = v.x, b = v.y, c = v.z;
    if (s >= 8) { a = c; b = 0; c = 0; } else if (s >= 4) { a = b; b = c; c = 0; }
    if (s >= 12) a = 0;
    const uint32_t sh = (uint32_t)(s & 3);
    orbx_uint3_u o;
    o.x = __builtin_amdgcn_alignbyte(b, a, sh); o.y = __builtin_amdgcn_alignbyte(c, b, sh); o.z = __builtin_amdgcn_alignbyte(0u, c, sh);
    return o;
}
// one in-place piece into its tile row: a row has 19 dwords, so the 7th piece is one dword, and none when the row is displaced by
// one dword (dsh = 1, first cell column)
__device__ __forceinline__ void fr_ip_store(uint32_t *d, const orbx_uint3_u &v, int dq, int dsh) {
    if (dq < 6) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }
    else if (dsh == 0) d[0] = v.x;
}
// INPLACE: the level-0 groups read the caller's grey image (`raw`) instead of the slab's padded level 0, which is not written
// in that mode: source rows through the reflection, the columns linearly; groups of the first / last cell column then mirror
// their (at most 3) ring columns inside the LDS tile.  Address arithmetic: orbx_inplace.h.  Every other level, and every
// instruction of the walk / ring test / NMS, is the same as in the slab form.
// (Two kernels, k_fast_rows and k_fast_rows_ip, share this body, so that the slab form keeps its name and its staging code; fr_nms's
// seam maxima are one 32-bit v_max3_u32 per side in every instance: the code object holds no three-input 16-bit min / max.)
// MODE: 0 = slab form (k_fast_rows), 1 = mixed (k_fast_rows_ip: the level-0 groups in place, the others from the slab), 2 = a
// launch of level-0 groups only, all in place (k_fast_rows_l0, the FAST-first plan of run_chunk): no slab staging path and no
// per-group level test.
template <int MODE>
__device__ __forceinline__ void fr_kernel(const DGeom &g, const OrbxCell *__restrict__ cells,
                                          const OrbxFastGroup *__restrict__ groups,
                                          const uint8_t *__restrict__ pyr, uint2 *__restrict__ cand,
                                          int *__restrict__ cand_cursor, int *__restrict__ status, int rows,
                                          int lcap, int ngroups, int gpw, int dbg_stop, int ccap, const OrbxRaw0 &raw) {
    // dbg_stop (ORBX_FAST_STOP, phase-timing builds only, -DORBX_TIMING_KNOBS; results are wrong unless 0): 1 = after
    // staging, 2 = after the pre-test, 3 = after the ring test, 4 = before NMS.  The shipped library pins it to 0.
#ifndef ORBX_TIMING_KNOBS
    dbg_stop = 0;
#endif
    constexpr bool INPLACE = MODE != 0, L0ONLY = MODE == 2;
    extern __shared__ __attribute__((aligned(16))) uint8_t fast_smem[];
    uint32_t *s_tile = (uint32_t *)fast_smem;
    // tile | score map (16-byte aligned: cleared with 16-byte stores) | work list (lcap entries + the re-run stack) |
    // corner list of the group (ccap entries: a group with more corners takes the dense NMS rescan)
    const FrLds lds = fr_lds(rows, lcap, ccap);
    uint8_t *s_score = fast_smem + lds.map_bytes;
    uint16_t *s_list = (uint16_t *)(fast_smem + lds.list_off);
    uint16_t *s_corn = (uint16_t *)(fast_smem + lds.corn_off);
    const int lane = threadIdx.x;
    const int f = blockIdx.x;   // frame fastest: all groups of one frame share one XCD's L2
    // One or two groups per wave (gpw; the handle refuses anything else), one after the other, as two PEELED trips of the group
    // body: the second group's tile is requested into a register set of its own once the first is staged, and nothing reads
    // those registers before the second group's staging, so its loads stay outstanding during walk, rounds and NMS of the
    // first.  (As a loop with the tile carried round it, the register allocator split the carried tuples and copied them out
    // at the loads: the wave waited for the whole tile before the first group's walk, profiles/prefetch_waits.md.)
    const int g0 = blockIdx.y * gpw;
    const int ng = min(gpw, ngroups - g0);
    // staging: a lane loads 12 bytes (one load, a third of the address arithmetic and of the load instructions of a
    // dword per lane), 7 lanes cover the 19 dwords of a tile row, 9 rows per step, 5 steps = 45 rows in registers.
    // Row offsets are 32-bit adds from the first row's offset, clamped to the cell's last row; the address is the
    // frame's scalar base + that 32-bit offset (global_load saddr form, no 64-bit vector arithmetic).  The lanes of a
    // row's last 12-byte piece read past the tile into the level's next bytes (the pyramid slab has slack at its end).
    const int rq = (lane * 37) >> 8, dq = lane - 7 * rq;   // lane / 7, lane % 7  (lane 63: rq = 9, idle)
    orbx_uint3_u tv_a[5], tv_b[5];   // the tiles of the wave's first and second group: two register sets, nothing loop-carried
    // (both groups' records up front -- a wave with one group reads its own twice: the second tile's request then hangs on no
    // chain of record loads, and no record load is retired behind it)
    const OrbxFastGroup grp_a = groups[g0], grp_b = groups[g0 + ng - 1];
    const OrbxCell c0_a = cells[grp_a.cell0], c1_a = cells[grp_a.cell0 + grp_a.ncell - 1];
    const OrbxCell c0_b = cells[grp_b.cell0], c1_b = cells[grp_b.cell0 + grp_b.ncell - 1];
    const uint8_t *fbase = pyr + (long long)f * g.pyr_bytes;
    const uint8_t *rbase = INPLACE ? raw.img + (long long)f * raw.frame_stride : nullptr;
    // the 45 register rows of group cn's tile, requested into tvn
    auto prefetch = [&](const OrbxCell &cn, orbx_uint3_u (&tvn)[5]) __attribute__((always_inline)) {
    if (L0ONLY || (INPLACE && cn.level == 0)) {
        int dsh_, shr_;
        const int xb_ = orbx_ip_fast_xb(cn.x0, &dsh_);
        const int col_ = orbx_ip_fast_piece_col(xb_, dq, raw.W, &shr_);
        const int ylast_ = (int)cn.y0 + (int)cn.ch - 1;
        if ((int)cn.y0 >= ORBX_EDGE && ylast_ - ORBX_EDGE < raw.H) {
            /* every cell row but the first and the last: no row is reflected, the offsets are the slab path's adds */
            uint32_t vstride9 = (uint32_t)(9 * raw.stride);
            asm("" : "+v"(vstride9));
            const uint32_t olast = orbx_ip_row_off(ylast_ - ORBX_EDGE, raw.stride, col_);
            uint32_t o = orbx_ip_row_off((int)cn.y0 - ORBX_EDGE + min(rq, 8), raw.stride, col_);
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                tvn[k] = *(const orbx_uint3_u *)(rbase + min(o, olast));
                o += vstride9;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int prow_ = min((int)cn.y0 + min(rq, 8) + 9 * k, ylast_);
                tvn[k] = *(const orbx_uint3_u *)(rbase + orbx_ip_row_off(orbx_ip_fast_row(prow_, raw.H), raw.stride, col_));
            }
        }
    } else {
        const DLevel &Ln = g.lv[cn.level];
        const uint8_t *srcn = fbase + Ln.off;
        uint32_t vpitch9 = (uint32_t)(9 * Ln.pitch);
        asm("" : "+v"(vpitch9));   /* in a VGPR: a VOP2 add with an SGPR source issues at the slow rate */
        const uint32_t olast = (uint32_t)(__mul24((int)cn.y0 + (int)cn.ch - 1, Ln.pitch) + (cn.x0 & ~3) + 12 * dq);
        uint32_t o = (uint32_t)(__mul24((int)cn.y0 + min(rq, 8), Ln.pitch) + (cn.x0 & ~3) + 12 * dq);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            tvn[k] = *(const orbx_uint3_u *)(srcn + min(o, olast));
            o += vpitch9;
        }
    }
    };
    prefetch(c0_a, tv_a);
  // one group: staged from its register set tv, walked, scored, thinned.  `first` (a std::bool_constant): the trip that requests the
  // wave's second tile, after its own is staged and before its walk
  auto group = [&](auto first, const OrbxFastGroup &grp, const OrbxCell &c0, const OrbxCell &c1,
                   const orbx_uint3_u (&tv)[5]) __attribute__((always_inline)) {
    const int level = L0ONLY ? 0 : (int)c0.level;
    const DLevel &L = g.lv[level];
    const int tw = c1.x0 + c1.cw - c0.x0, th_rows = c0.ch;
    const int niw = tw - 6;                                   // interior columns of the group (<= 64)
    const int iw0 = grp.ncell == 2 ? c0.cw - 6 : 64;
    // ---- stage the tile: prefetched registers -> LDS
    const bool ip0 = L0ONLY || (INPLACE && c0.level == 0);   // wave-uniform
    if (ip0) {
        int dsh, shr;
        const int xb = orbx_ip_fast_xb(c0.x0, &dsh);
        const int col = orbx_ip_fast_piece_col(xb, dq, raw.W, &shr);
        const bool clamped = xb + 84 > raw.W;    // some piece of this group was loaded from W - 12
        uint32_t *trow = s_tile + rq * (FR_TP / 4) + 3 * dq + dsh;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            if (rq < 9 && 9 * k + rq < th_rows) {
                uint32_t *d = trow + 9 * k * (FR_TP / 4);
                fr_ip_store(d, clamped ? orbx_shr96(tv[k], shr) : tv[k], dq, dsh);
            }
        }
        if (th_rows > 45) {
            for (int r = 45 + rq; r < th_rows; r += 9) {
                if (rq < 9) {
                    orbx_uint3_u v = *(const orbx_uint3_u *)(rbase + orbx_ip_row_off(orbx_ip_fast_row((int)c0.y0 + r, raw.H), raw.stride, col));
                    if (clamped) v = orbx_shr96(v, shr);
                    fr_ip_store(s_tile + r * (FR_TP / 4) + 3 * dq + dsh, v, dq, dsh);
                }
            }
        }
        // ring columns: raw columns < 0 (first cell column) and >= W (last cell column) mirror columns of the tile itself
        const int rs = (int)c0.x0 - ORBX_EDGE;
        const int nl = rs < 0 ? -rs : 0, nr = max(rs + tw - raw.W, 0);
        if (nl + nr > 0) {
            orbx_wave_sync();
            uint8_t *t8 = (uint8_t *)s_tile;
            const int p0 = 4 * dsh - xb, pW = p0 + raw.W;   // LDS bytes of raw columns 0 and W
            for (int r = lane; r < th_rows; r += 64) {
                uint8_t *row = t8 + r * FR_TP;
                for (int i = 1; i <= nl; ++i) row[p0 - i] = row[p0 + i];
                for (int i = 0; i < nr; ++i) row[pW + i] = row[pW - 2 - i];
            }
        }
    } else {
        const int xa = c0.x0 & ~3;
        uint32_t *trow = s_tile + rq * (FR_TP / 4) + 3 * dq;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            if (rq < 9 && 9 * k + rq < th_rows) {
                uint32_t *d = trow + 9 * k * (FR_TP / 4);
                d[0] = tv[k].x;
                if (dq < 6) { d[1] = tv[k].y; d[2] = tv[k].z; }   // a row has 19 dwords: the 7th piece is one dword
            }
        }
        if (th_rows > 45) {   // cells taller than the register window (tiny pyramid levels only)
            const uint8_t *src = fbase + L.off + (long long)c0.y0 * L.pitch + xa + 12 * dq;
            for (int r = 45 + rq; r < th_rows; r += 9) {
                if (rq < 9) {
                    const orbx_uint3_u v = *(const orbx_uint3_u *)(src + (long long)r * L.pitch);
                    uint32_t *d = s_tile + r * (FR_TP / 4) + 3 * dq;
                    d[0] = v.x;
                    if (dq < 6) { d[1] = v.y; d[2] = v.z; }
                }
            }
        }
    }
    // score map cleared with 16-byte stores (the launcher rounds the row count to a multiple of 4, so the map is
    // 16-byte aligned and a few bytes past the cell's last row still belong to it or to the not-yet-used list)
    for (int i = lane; i < (th_rows * (FR_TP / 4) + 3) / 4; i += 64) ((uint4 *)s_score)[i] = make_uint4(0, 0, 0, 0);
    if constexpr (decltype(first)::value) {
        // Every load so far is retired HERE, on every path (a wave with one group included: the paths join again below):
        // s_waitcnt vmcnt(0), gfx9 encoding, expcnt and lgkmcnt left at their maxima.  The wave has consumed its tile, so this
        // waits for nothing, but the staging stores and the loads of the extra rows sit in divergent branches, and on the paths
        // around them the compiler's wait bookkeeping keeps those loads outstanding: the first reuse of one of their registers
        // in the walk would then wait for them -- and for the second tile's loads, which are younger, with them.
        __builtin_amdgcn_s_waitcnt(0x0F70);
        if (ng > 1) prefetch(c0_b, tv_b);
    }
    FrCtx cx;
    cx.tile = (const uint8_t *)s_tile + (ip0 ? orbx_ip_fast_tile_off(c0.x0) : (c0.x0 & 3));
    cx.score = s_score;
    cx.list = s_list;
    cx.corn = s_corn;
    cx.lcap = lcap;
    cx.lane = lane;
    FrCells gc;
    gc.iw0 = iw0;
    gc.offx0 = c0.offx; gc.offx1 = c1.offx; gc.offy = c0.offy;
    gc.ord0 = c0.idx_in_level; gc.ord1 = c1.idx_in_level;
    gc.cap0 = c0.slot_cap; gc.cap1 = c1.slot_cap;
    gc.out = cand + (long long)f * g.cand_total + L.cand_begin;
    gc.cursor = cand_cursor + f * g.nlevels + level;
    gc.out_cap = L.cand_cap;
    orbx_wave_sync();
    if (dbg_stop == 1) return;
    const bool two_th = g.min_th != g.ini_th;
    const bool colv = lane < niw;
    const bool second = lane >= iw0;
    const uint8_t *pc = cx.tile + 3 + (colv ? lane : 0);   // this lane's column, row 0
    const int yend = th_rows - 3;
    int ns0 = 0, ns1 = 0;
    unsigned act = grp.ncell == 2 ? 3u : 1u;   // cells still to be detected in this pass
    for (int pass = 0; pass < 2; ++pass) {
        const int th = pass == 0 ? g.ini_th : g.min_th;
        const bool lane_on = colv && ((act >> (second ? 1 : 0)) & 1u);
        int nctot = 0;
        bool overflow = false;
        int y = 3;
        // lanes that are switched off (outside the group, or a cell that already has keypoints) carry a threshold no
        // 8-bit difference reaches: the pre-test needs no separate lane mask
        const fr_i16 thv = lane_on ? (fr_i16)th : (fr_i16)0x4000;
        // A pair of cells may be up to ORBX_FAST_XCOLS columns wider than the wave (two 33-column cells: level 2 and 5 of 640x480 would
        // otherwise run one cell per wave, half the lanes idle; ORBX_FAST_XCOLS).  The row walk covers columns 0..63; the columns beyond are
        // tested afterwards with the lanes as ROWS, one column per step, into the same work list.
        int xc = 64;
        const fr_i16 thx = (colx_on_mask(act) && 3 + lane < yend) ? (fr_i16)th : (fr_i16)0x4000;
        while (y < yend || xc < niw) {
            // ---- compass pre-test, one row per step: a 9-arc of the 16-ring contains one pixel of every opposite
            // pair, so max(min(max(r0,r8),max(r4,r12)) - v, v - max(min(r0,r8),min(r4,r12))) > th is necessary.
            // The column window (rows y-3 .. y+3) rotates through seven registers: one new LDS byte per row.
            // Scalar instructions issue at the same rate as vector ones, so the step is written to need only two
            // (popcount + list cursor): no per-row exit test, the lane mask folded into the threshold; the list store is
            // the step's one exec-masked instruction (the select of a dummy slot in its place takes one v_mov per row
            // more, profiles/r03_fast_onepass.md).
            const uint8_t *pr = pc + y * FR_TP;
            fr_u16 w0 = pr[-3 * FR_TP], w1 = pr[-2 * FR_TP], w2 = pr[-FR_TP], w3 = pr[0], w4 = pr[FR_TP], w5 = pr[2 * FR_TP], w6;
            // list cursor as an LDS byte ADDRESS (scalar): a lane's slot is one v_lshl_add away
            const uint32_t list0 = (uint32_t)(uintptr_t)(fr_lds_u16 *)s_list;
            uint32_t nb = list0;
            uint32_t code = (uint32_t)((y << 8) | lane);
            // software-pipelined: the three LDS bytes of row y+1 are requested before row y is evaluated (the list
            // store could alias them as far as the compiler knows, so it would not hoist them itself); the row after
            // the last one is read but never used (it is the first row of the score map)
            uint32_t nx0 = pr[3 * FR_TP], nx4 = pr[3], nx12 = pr[-3];   // (32-bit carriers: no re-extension in the loop)
#define FR_STEP(R8, C, R0)                                                                                              \
            {                                                                                                           \
                R0 = (fr_u16)nx0;                                                                                       \
                const fr_u16 r4 = (fr_u16)nx4, r12 = (fr_u16)nx12;                                                      \
                pr += FR_TP;                                                                                            \
                nx0 = pr[3 * FR_TP]; nx4 = pr[3]; nx12 = pr[-3];                                                        \
                asm("" : "+v"(nx0), "+v"(nx4), "+v"(nx12));   /* keeps the carriers 32-bit (no v_and / SDWA re-extension) */ \
                const fr_u16 A = fr_min(fr_max(R0, R8), fr_max(r4, r12));                                               \
                const fr_u16 Bm = fr_max(fr_min(R0, R8), fr_min(r4, r12));                                              \
                const bool cnd = fr_smax((fr_i16)(A - C), (fr_i16)(C - Bm)) > thv;                                      \
                const unsigned long long m = orbx_ballot(cnd);                                                          \
                if (cnd) *(fr_lds_u16 *)(uintptr_t)(nb + 2u * (uint32_t)orbx_wave_rank(m)) = (uint16_t)code;           \
                { const uint32_t pc_ = (uint32_t)__popcll(m);                                                           \
                  asm("s_lshl1_add_u32 %0, %1, %0" : "+s"(nb) : "s"(pc_) : "scc"); }   /* nb += 2 * popcount: ONE scalar instruction, ONE scalar cursor (a lane's slot stays mbcnt, mbcnt, v_lshl_add) */ \
                code += 0x100u;                                                                                         \
            }
            // full chunks of 7 rows while the list is guaranteed to take them
            while (y + 7 <= yend && nb + 7u * 128u <= list0 + 2u * (uint32_t)lcap) {
                FR_STEP(w0, w3, w6)
                FR_STEP(w1, w4, w0)
                FR_STEP(w2, w5, w1)
                FR_STEP(w3, w6, w2)
                FR_STEP(w4, w0, w3)
                FR_STEP(w5, w1, w4)
                FR_STEP(w6, w2, w5)
                y += 7;
            }
            // remaining rows (and small work lists) one at a time, shifting the window
            while (y < yend && nb + 128u <= list0 + 2u * (uint32_t)lcap) {
                FR_STEP(w0, w3, w6)
                w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; w5 = w6;
                ++y;
            }
#undef FR_STEP
            // the columns beyond the wave (rows done): lane = row 3 + lane, one column per step while the list takes 64 more
            while (y >= yend && xc < niw && nb + 128u <= list0 + 2u * (uint32_t)lcap) {
                const uint8_t *px = cx.tile + (3 + lane) * FR_TP + 3 + xc;
                const fr_u16 C = px[0], r0 = px[-3 * FR_TP], r8 = px[3 * FR_TP], r4 = px[3], r12 = px[-3];
                const fr_u16 A = fr_min(fr_max(r0, r8), fr_max(r4, r12));
                const fr_u16 Bm = fr_max(fr_min(r0, r8), fr_min(r4, r12));
                const bool cnd = fr_smax((fr_i16)(A - C), (fr_i16)(C - Bm)) > thx;
                const unsigned long long m = orbx_ballot(cnd);
                if (cnd) *(fr_lds_u16 *)(uintptr_t)(nb + 2u * (uint32_t)orbx_wave_rank(m)) = (uint16_t)(((3 + lane) << 8) | xc);
                nb += 2u * (uint32_t)__popcll(m);
                ++xc;
            }
            const int n = (int)((nb - list0) >> 1);
            orbx_wave_sync();
            if (dbg_stop == 2) { if (n == 12345) cand_cursor[0] = n; continue; }
            const int ncorn = fr_ring_and_score(cx, n, th);
            // keep the corners for the NMS walk while they fit
            if (!overflow && nctot + ncorn <= ccap) {
                for (int e = lane; e < ncorn; e += 64) s_corn[nctot + e] = s_list[e];
                nctot += ncorn;
            } else {
                overflow = true;
            }
            orbx_wave_sync();
        }
        // ---- NMS
        int a0 = 0, a1 = 0;
        if (dbg_stop >= 2) { a0 = a1 = 1; } else
        if (!overflow) {
            fr_nms(cx, gc, s_corn, nctot, a0, a1);
        } else {
            int xs = 64;
            for (int yy = 3; yy < yend || xs < niw;) {
                int n = 0;
                for (; yy < yend && n + 64 <= lcap; ++yy) {
                    const bool cnd = lane_on && s_score[yy * FR_TP + 3 + lane] != 0;
                    const unsigned long long m = orbx_ballot(cnd);
                    if (cnd) s_list[n + orbx_wave_rank(m)] = (uint16_t)((yy << 8) | lane);
                    n += __popcll(m);
                }
                for (; yy >= yend && xs < niw && n + 64 <= lcap; ++xs) {   // columns beyond the wave: lane = row
                    const bool cnd = colx_on_mask(act) && 3 + lane < yend && s_score[(3 + lane) * FR_TP + 3 + xs] != 0;
                    const unsigned long long m = orbx_ballot(cnd);
                    if (cnd) s_list[n + orbx_wave_rank(m)] = (uint16_t)(((3 + lane) << 8) | xs);
                    n += __popcll(m);
                }
                orbx_wave_sync();
                fr_nms(cx, gc, s_list, n, a0, a1);
                orbx_wave_sync();
            }
        }
        if (act & 1u) ns0 = a0;
        if (act & 2u) ns1 = a1;
        if (pass == 1 || !two_th) break;
        // vKeysCell.empty() -> that cell alone repeats with minThFAST (:1519-1527)
        act = (ns0 == 0 ? 1u : 0u) | ((grp.ncell == 2 && ns1 == 0) ? 2u : 0u);
        if (act == 0) break;
        orbx_wave_sync();
        // score map cleared with 16-byte stores (the launcher rounds the row count to a multiple of 4, so the map is
        // 16-byte aligned and a few bytes past the cell's last row still belong to it or to the not-yet-used list)
        for (int i = lane; i < (th_rows * (FR_TP / 4) + 3) / 4; i += 64) ((uint4 *)s_score)[i] = make_uint4(0, 0, 0, 0);
        orbx_wave_sync();
    }
    // more survivors than the cell may report (only when max_cand_per_cell cut the exact worst case): reported, not silent
    if (lane == 0 && (ns0 > gc.cap0 || (grp.ncell == 2 && ns1 > gc.cap1))) atomicMax(&status[f], (int)ORBX_CAPACITY);
    orbx_wave_sync();   // the next group overwrites tile / score / lists
  };
    group(std::true_type{}, grp_a, c0_a, c1_a, tv_a);
    if (ng > 1) group(std::false_type{}, grp_b, c0_b, c1_b, tv_b);
}
__global__ __launch_bounds__(64, FR_WPS) void k_fast_rows(DGeom g, const OrbxCell *__restrict__ cells,
                                                          const OrbxFastGroup *__restrict__ groups,
                                                          const uint8_t *__restrict__ pyr, uint2 *__restrict__ cand,
                                                          int *__restrict__ cand_cursor, int *__restrict__ status, int rows,
                                                          int lcap, int ngroups, int gpw, int dbg_stop, int ccap) {
    const OrbxRaw0 none = {nullptr, 0, 0, 0, 0};
    fr_kernel<0>(g, cells, groups, pyr, cand, cand_cursor, status, rows, lcap, ngroups, gpw, dbg_stop, ccap, none);
}
__global__ __launch_bounds__(64, FR_WPS) void k_fast_rows_ip(DGeom g, const OrbxCell *__restrict__ cells,
                                                             const OrbxFastGroup *__restrict__ groups,
                                                             const uint8_t *__restrict__ pyr, uint2 *__restrict__ cand,
                                                             int *__restrict__ cand_cursor, int *__restrict__ status, int rows,
                                                             int lcap, int ngroups, int gpw, int dbg_stop, int ccap, OrbxRaw0 raw) {
    fr_kernel<1>(g, cells, groups, pyr, cand, cand_cursor, status, rows, lcap, ngroups, gpw, dbg_stop, ccap, raw);
}
__global__ __launch_bounds__(64, FR_WPS) void k_fast_rows_l0(DGeom g, const OrbxCell *__restrict__ cells,
                                                             const OrbxFastGroup *__restrict__ groups, uint2 *__restrict__ cand,
                                                             int *__restrict__ cand_cursor, int *__restrict__ status, int rows,
                                                             int lcap, int ngroups, int gpw, int dbg_stop, int ccap, OrbxRaw0 raw) {
    fr_kernel<2>(g, cells, groups, nullptr, cand, cand_cursor, status, rows, lcap, ngroups, gpw, dbg_stop, ccap, raw);
}

// ------------------------------------------------------------------------------------------------
// K3: DistributeOctTree (reference src/ORBextractor.cc:1050-1417) -- one workgroup per (frame, level).
//
// The reference mutates a std::list sequentially; its observable result (which nodes exist, their list
// order, which key each keeps) is reproduced here by level-synchronous passes:
//   * a key never moves: it only carries the list position of its node (knode[k]);
//   * one pass = every expandable node counts its 4 quadrants with LDS atomics, then a prefix scan over the
//     list gives each child its creation rank r; push_front order means child r lands at position C-1-r
//     and surviving old nodes follow in their old relative order;
//   * the "careful" phase (:1284-1375) sorts the expandable nodes by (count, creation order) and splits the
//     largest first until the list holds N nodes: all candidates are split speculatively, a scan over the
//     sorted order finds the cut, and only the nodes before the cut are materialised;
//   * the address tie-break of std::sort over pair<int,ExtractorNode*> is defined as creation order (F3).
// Selection (:1387-1413) = max response, first in emission order, via one 64-bit LDS atomicMax per key.
//
// Where a key lives (workgroup-uniform, K = the level's candidates, T = workgroup size):
//   K <= reg_keys * T   registers: thread tid owns keys tid + j * T, j < QT_KPT (position word, node index, stage B's quadrant);
//   K <= lds_keys       LDS key slots kpos_lds / knode_lds;
//   otherwise           positions re-read from the dense array, key -> node map in global scratch (knode_glob).
// kpos / knode of a key are only ever touched by the thread that owns it, on every path.
//
// Stages of one pass (one barrier after each; DESIGN.md section 5 has the measurements behind the list):
//   B  census: every key of a node that splits (F) counts itself into its quadrant (LDS atomics; per wave with ballots while
//      the list is one node, register path: QT_CENSUS_NODES);
//   C  ranks: main pass -- one two-word scan over the list (qt_scan_main); careful pass -- sort, speculative split, cut;
//   D  the next list is built (children in push_front order, survivors behind them); F of a child = more than one key;
//   E  keys follow their node; the next list's quadrant counters are zeroed in the same interval.
// There is no stage that decides which nodes split: F is written where a node is created.  The list size is ctot + nmtot,
// which every thread holds.
// ------------------------------------------------------------------------------------------------
// Workgroup size is a template parameter, picked per launch (orbx_launch_quadtree): the kernel is a chain of barrier-separated
// stages, so many small workgroups win when the launch has several workgroups per CU to choose from (256 threads: 67 us per
// 256 frames of 640x480 / 1000 features against 82 us with 512), and large ones when there are few workgroups with many keys
// each (1920x1080 / 4000 features, 32 frames = one workgroup per CU: 185 / 112 / 82 us with 256 / 512 / 1024 threads).

struct QtShared {
    int size, jstar, m, pad;
    uint32_t wsum[16];    // one per wave, up to 1024 threads
    uint32_t wsum2[16];   // second word of qt_scan_main
};
static_assert(sizeof(QtShared) <= QT_SHARED_BYTES, "QtShared outgrew its LDS slot");

// exclusive prefix sum of in[0..n) -> out[0..n) (both LDS, may alias), returns total; all threads must call.
// Two barriers per 512-element chunk: wave scan -> wave totals in LDS -> every thread adds the totals before it.
template <int QT_THREADS>
__device__ uint32_t qt_block_scan(const uint32_t *in, uint32_t *out, int n, QtShared *sh) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t carry = 0;
    for (int base = 0; base < n; base += QT_THREADS) {
        const int i = base + tid;
        const uint32_t v = i < n ? in[i] : 0;
        const uint32_t incl = (uint32_t)orbx_wave_scan((int)v);
        if (lane == 63) sh->wsum[w] = incl;
        __syncthreads();
        uint32_t off = carry, tot = 0;
#pragma unroll
        for (int j = 0; j < QT_THREADS / 64; ++j) {
            const uint32_t t = sh->wsum[j];
            off += j < w ? t : 0u;
            tot += t;
        }
        if (i < n) out[i] = off + incl - v;
        carry += tot;
        __syncthreads();   // results visible to every thread; wsum free for the next chunk / call
    }
    return carry;
}

// Main-pass creation ranks in ONE scan over the list, inputs computed on the fly from the census:
//   word a = children (low 16) | expandable children (high 16) of an expandable node, word b = 1 for a survivor.
// t1[p] / t2[p] get the exclusive sums, the totals come back in tot_a / tot_b.  Entry p is written by the thread that
// reads it again in stage D (p = tid + i * QT_THREADS in both), so no barrier follows the last chunk: one barrier per chunk
// plus one between chunks (wsum reuse).  The next writer of wsum is a scan of the next pass, at least two barriers later.
template <int QT_THREADS>
__device__ __forceinline__ void qt_scan_main(const uint32_t *meta, const uint32_t *cc, uint32_t *t1, uint32_t *t2, int n,
                                             QtShared *sh, uint32_t &tot_a, uint32_t &tot_b) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t carry_a = 0, carry_b = 0;
    for (int base = 0; base < n; base += QT_THREADS) {
        const int i = base + tid;
        uint32_t a = 0, b = 0;
        if (i < n) {
            if ((meta[i] >> 16) & 1) {
                const uint4 c = *(const uint4 *)(cc + 4 * i);
                const uint32_t ne = (c.x > 0) + (c.y > 0) + (c.z > 0) + (c.w > 0);
                const uint32_t nx = (c.x > 1) + (c.y > 1) + (c.z > 1) + (c.w > 1);
                a = ne | (nx << 16);
            } else b = 1;
        }
        const uint32_t ia = (uint32_t)orbx_wave_scan((int)a), ib = (uint32_t)orbx_wave_scan((int)b);
        if (lane == 63) { sh->wsum[w] = ia; sh->wsum2[w] = ib; }
        __syncthreads();
        uint32_t offa = carry_a, offb = carry_b, ta = 0, tb = 0;
#pragma unroll
        for (int j = 0; j < QT_THREADS / 64; ++j) {
            const uint32_t xa = sh->wsum[j], xb = sh->wsum2[j];
            offa += j < w ? xa : 0u;  ta += xa;
            offb += j < w ? xb : 0u;  tb += xb;
        }
        if (i < n) { t1[i] = offa + ia - a; t2[i] = offb + ib - b; }
        carry_a += ta; carry_b += tb;
        if (base + QT_THREADS < n) __syncthreads();
    }
    tot_a = carry_a; tot_b = carry_b;
}

__device__ __forceinline__ int qt_quadrant(uint32_t pos, uint32_t b0, uint32_t b1) {
    const int x = pos & 0xfff, y = (pos >> 12) & 0xfff;
    const int x0 = b0 & 0xffff, y0 = b0 >> 16, x1 = b1 & 0xffff, y1 = b1 >> 16;
    const int mx = x0 + ((x1 - x0 + 1) >> 1), my = y0 + ((y1 - y0 + 1) >> 1);  // ceil(d/2), DivideNode :968-969
    return (x < mx ? 0 : 1) + (y < my ? 0 : 2);
}

__device__ __forceinline__ void qt_child_box(uint32_t b0, uint32_t b1, int q, uint32_t &c0, uint32_t &c1) {
    const int x0 = b0 & 0xffff, y0 = b0 >> 16, x1 = b1 & 0xffff, y1 = b1 >> 16;
    const int mx = x0 + ((x1 - x0 + 1) >> 1), my = y0 + ((y1 - y0 + 1) >> 1);
    const int cx0 = (q & 1) ? mx : x0, cx1 = (q & 1) ? x1 : mx;
    const int cy0 = (q & 2) ? my : y0, cy1 = (q & 2) ? y1 : my;
    c0 = (uint32_t)cx0 | ((uint32_t)cy0 << 16);
    c1 = (uint32_t)cx1 | ((uint32_t)cy1 << 16);
}

// One workgroup's whole problem.  KEYS_IN_REG is the register path (K <= reg_keys * QT_THREADS, decided by the kernel): it is
// a template parameter and not a run-time flag so that each copy of the pass loop keeps only its own addresses and keys live.
template <int QT_THREADS, bool KEYS_IN_REG>
__device__ __forceinline__ void qt_workgroup(const DGeom &g, const uint2 *__restrict__ dense_all,
                                             const int *__restrict__ cand_count,
                                             uint32_t *__restrict__ lvl_kp, int *__restrict__ lvl_count,
                                             int *__restrict__ status, uint16_t *__restrict__ knode_glob,
                                             int ncap, int lds_keys, int level_begin) {
    extern __shared__ __attribute__((aligned(16))) uint8_t qt_smem[];
    // grid: frame fastest, level 0 (the most keys) dispatched first.  With the level fastest, workgroup id % 8 = level for
    // the usual 8 levels: one XCD would get every level-0 workgroup and another every level-7 one.
    const int level = level_begin + blockIdx.y, f = blockIdx.x, tid = threadIdx.x;
    const DLevel &L = g.lv[level];
    const int N = L.nfeat;
    const uint2 *cand = dense_all + (long long)f * g.cand_total + L.cand_begin;
    // ---- LDS carve-up (all arrays have ncap entries unless noted)
    uint8_t *sp = qt_smem;
    QtShared *sh = (QtShared *)sp;                 sp += QT_SHARED_BYTES;
    uint32_t *boxA0 = (uint32_t *)sp;              sp += 4 * (size_t)ncap;
    uint32_t *boxA1 = (uint32_t *)sp;              sp += 4 * (size_t)ncap;
    uint32_t *cntA = (uint32_t *)sp;               sp += 4 * (size_t)ncap;
    uint32_t *metaA = (uint32_t *)sp;              sp += 4 * (size_t)ncap;   // crank | F << 16
    uint32_t *boxB0 = (uint32_t *)sp;              sp += 4 * (size_t)ncap;
    uint32_t *boxB1 = (uint32_t *)sp;              sp += 4 * (size_t)ncap;
    uint32_t *cntB = (uint32_t *)sp;               sp += 4 * (size_t)ncap;
    uint32_t *metaB = (uint32_t *)sp;              sp += 4 * (size_t)ncap;
    uint32_t *cc = (uint32_t *)sp;                 sp += 16 * (size_t)ncap;  // [ncap][4] quadrant counts
    unsigned long long *best = (unsigned long long *)cc;                      // selection keys: the quadrant counts are dead by then
    uint16_t *newpos = (uint16_t *)sp;             sp += 8 * (size_t)ncap + 16;  // [ncap][4] child list positions (< ncap); [p][0] for survivors
    uint32_t *t0 = (uint32_t *)sp;                 sp += 4 * (size_t)ncap;   // scan input
    uint32_t *t1 = (uint32_t *)sp;                 sp += 4 * (size_t)ncap;   // scan output E
    uint32_t *t2 = (uint32_t *)sp;                 sp += 4 * (size_t)ncap;   // scan output NM
    uint32_t *t3 = (uint32_t *)sp;                 sp += 4 * (size_t)ncap;   // careful: rank / by-rank data
    uint32_t *t4 = (uint32_t *)sp;                 sp += 4 * (size_t)ncap;
    uint32_t *t5 = (uint32_t *)sp;                 sp += 4 * (size_t)ncap;
    uint32_t *kpos_lds = (uint32_t *)sp;           sp += 4 * (size_t)lds_keys;  // key positions (x:12 y:12 score:8) when K <= lds_keys
    uint16_t *knode_lds = (uint16_t *)sp;
    uint32_t *box0 = boxA0, *box1 = boxA1, *cnt = cntA, *meta = metaA;
    uint32_t *nbox0 = boxB0, *nbox1 = boxB1, *ncnt = cntB, *nmeta = metaB;

    // ---- keys: k_fast_rows appended this level's survivors to the dense array (count in cand_count); nothing to gather
    const int K = min(cand_count[f * g.nlevels + level], L.cand_cap);
    // workgroup-uniform: thread tid owns keys tid + j * QT_THREADS, j < QT_KPT, and keeps each one's position word and
    // node index (low 16; the quadrant of stage B above them) in registers.  Every loop over j is fully unrolled, so the
    // arrays are registers, not scratch; a slot without a key (k >= K) holds node 0 and is never used.
    constexpr bool keys_in_reg = KEYS_IN_REG;
    uint32_t rpos[QT_KPT], rnode[QT_KPT];
#pragma unroll
    for (int j = 0; j < QT_KPT; ++j) {
        const int k = tid + j * QT_THREADS;
        rpos[j] = keys_in_reg && k < K ? cand[k].x : 0u;
        rnode[j] = 0;
    }
    const bool keys_in_lds = !keys_in_reg && K <= lds_keys;   // workgroup-uniform: key positions and key->node map live in LDS
    if (keys_in_lds)
        for (int k = tid; k < K; k += QT_THREADS) kpos_lds[k] = cand[k].x;
    uint16_t *knode = keys_in_lds ? knode_lds : knode_glob + ((long long)f * g.cand_total + L.cand_begin);
#define QT_KPOS(k) (keys_in_lds ? kpos_lds[k] : cand[k].x)
    __syncthreads();
    // ---- roots (:1060-1135)
    const int nini = L.nini;
    const float hx = L.hx;
    for (int i = tid; i < nini; i += QT_THREADS) cc[i] = 0;
    __syncthreads();
    if (keys_in_reg) {
        const bool census = QT_CENSUS_NODES > 0 && nini <= 4;   // every key of the wave hits one of nini counters: count per wave
#pragma unroll
        for (int j = 0; j < QT_KPT; ++j)
            if (tid + j * QT_THREADS < K) {
                const int b = min((int)((float)(rpos[j] & 0xfff) / hx), nini - 1);
                rnode[j] = (uint32_t)b;
                if (!census) atomicAdd(&cc[b], 1u);
            }
        if (census)
            for (int b = 0; b < nini; ++b) {
                uint32_t n = 0;
#pragma unroll
                for (int j = 0; j < QT_KPT; ++j) n += __popcll(orbx_ballot(tid + j * QT_THREADS < K && rnode[j] == (uint32_t)b));
                if ((tid & 63) == 0 && n) atomicAdd(&cc[b], n);
            }
    } else
    for (int k = tid; k < K; k += QT_THREADS) {
        const int x = QT_KPOS(k) & 0xfff;
        int b = (int)((float)x / hx);
        b = min(b, nini - 1);
        knode[k] = (uint16_t)b;
        atomicAdd(&cc[b], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int i = 0; i < nini; ++i) {
            if (cc[i] > 0) {
                box0[n] = (uint32_t)(int)(hx * (float)i);                       // UL.x | UL.y(=0) << 16
                box1[n] = (uint32_t)(int)(hx * (float)(i + 1)) | ((uint32_t)L.qt_h << 16);
                cnt[n] = cc[i];
                meta[n] = (uint32_t)(cc[i] > 1) << 16;   // F: splits in the first pass
                t0[i] = n++;
            } else t0[i] = 0xffff;
        }
        sh->size = n;
    }
    __syncthreads();
    if (keys_in_reg) {
#pragma unroll
        for (int j = 0; j < QT_KPT; ++j) rnode[j] = tid + j * QT_THREADS < K ? t0[rnode[j]] : 0u;
    } else
    for (int k = tid; k < K; k += QT_THREADS) knode[k] = (uint16_t)t0[knode[k]];
    int size = sh->size;
    // the root counts in cc are dead (thread 0 read them before the barrier above): zero the first pass's quadrant counters
    for (int p = tid; p < size; p += QT_THREADS) *(uint4 *)(cc + 4 * p) = make_uint4(0, 0, 0, 0);
    __syncthreads();

    bool careful = false;
    while (size > 0) {
        // ---- B: quadrant census of the nodes that split in this pass (F).  F is what the pass that created the node wrote:
        //      a root or a child with more than one key; a survivor has at most one (main phase) or was not created by the
        //      last pass (careful phase), F = 0.  The counters were zeroed in the barrier interval of the previous stage E.
        if (keys_in_reg) {
            const bool census = QT_CENSUS_NODES > 0 && size <= QT_CENSUS_NODES;   // few nodes: hundreds of keys on 4 * size counters, counted per wave below
            // the node reads of QT_BGRP keys are issued before any is used (all QT_KPT at once cost registers that the
            // 8 waves per SIMD of the 256-thread workgroup do not have)
#pragma unroll
            for (int j0 = 0; j0 < QT_KPT; j0 += QT_BGRP) {
                uint32_t m[QT_BGRP], b0[QT_BGRP], b1[QT_BGRP];
#pragma unroll
                for (int i = 0; i < QT_BGRP; ++i) { const int p = rnode[j0 + i]; m[i] = meta[p]; b0[i] = box0[p]; b1[i] = box1[p]; }
#pragma unroll
                for (int i = 0; i < QT_BGRP; ++i)
                    if (tid + (j0 + i) * QT_THREADS < K && ((m[i] >> 16) & 1)) {
                        const int p = rnode[j0 + i], q = qt_quadrant(rpos[j0 + i], b0[i], b1[i]);
                        if (!census) atomicAdd(&cc[4 * p + q], 1u);
                        rnode[j0 + i] = (uint32_t)p | ((uint32_t)q << 16) | 0x80000000u;   // stage E reuses the quadrant; bit 31: counted
                    }
            }
            if (census)
                for (int c = 0; c < 4 * size; ++c) {
                    const uint32_t code = 0x80000000u | (uint32_t)(c >> 2) | ((uint32_t)(c & 3) << 16);
                    uint32_t n = 0;
#pragma unroll
                    for (int j = 0; j < QT_KPT; ++j) n += __popcll(orbx_ballot(rnode[j] == code));
                    if ((tid & 63) == 0 && n) atomicAdd(&cc[c], n);
                }
        } else
        for (int k = tid; k < K; k += QT_THREADS) {
            const int p = knode[k];
            if ((meta[p] >> 16) & 1) atomicAdd(&cc[4 * p + qt_quadrant(QT_KPOS(k), box0[p], box1[p])], 1u);
        }
        __syncthreads();
        // ---- C: creation ranks
        int ctot, nmtot, nexp_total = 0;
        if (!careful) {
            uint32_t tot, nm;
            qt_scan_main<QT_THREADS>(meta, cc, t1, t2, size, sh, tot, nm);
            ctot = tot & 0xffff;
            nexp_total = tot >> 16;
            nmtot = (int)nm;
        } else {
            // careful phase: order candidates by descending (count, creation rank).  The candidate keys are first
            // compacted into a dense, 16-byte aligned LDS array (scratch = newpos, rewritten in phase D anyway); each
            // candidate then counts the larger keys with ds_read_b128 over M/4 steps instead of walking the whole list.
            uint32_t *dk = (uint32_t *)newpos, *dp = dk + (size_t)ncap + 4;   // dense keys [M + 4], back references [M]: 8 ncap + 16 bytes
            for (int p = tid; p < size; p += QT_THREADS) { t0[p] = (meta[p] >> 16) & 1; t3[p] = 0xffffffffu; }
            __syncthreads();
            const int Mc = (int)qt_block_scan<QT_THREADS>(t0, t1, size, sh);
            for (int p = tid; p < size; p += QT_THREADS)
                if ((meta[p] >> 16) & 1) { dk[t1[p]] = (cnt[p] << 16) | (meta[p] & 0xffffu); dp[t1[p]] = p; }
            if (tid < 4) dk[Mc + tid] = 0u;   // padding compares as "not larger"
            __syncthreads();
            for (int i = tid; i < Mc; i += QT_THREADS) {
                const uint32_t key = dk[i];
                uint32_t rank = 0;
                for (int j = 0; j < Mc; j += 4) {
                    const uint4 v = *(const uint4 *)(dk + j);
                    rank += (v.x > key) + (v.y > key) + (v.z > key) + (v.w > key);
                }
                t3[dp[i]] = rank;
            }
            if (tid == 0) { sh->m = 0; sh->jstar = 0x7fffffff; }
            __syncthreads();
            // scatter (children, children-1) by rank
            for (int p = tid; p < size; p += QT_THREADS) {
                if (t3[p] != 0xffffffffu) {
                    uint32_t ne = 0;
                    for (int q = 0; q < 4; ++q) ne += cc[4 * p + q] > 0;
                    t4[t3[p]] = ne | ((ne - 1) << 16);
                    atomicAdd(&sh->m, 1);
                }
            }
            __syncthreads();
            const int M = sh->m;
            qt_block_scan<QT_THREADS>(t4, t5, M, sh);  // exclusive, packed: CE (low 16) | sum(ne-1) before (high 16)
            for (int r = tid; r < M; r += QT_THREADS) {
                const int after = size + (int)(t5[r] >> 16) + (int)(t4[r] >> 16);  // list size after splitting rank r
                if (after >= N) atomicMin(&sh->jstar, r);
            }
            __syncthreads();
            const int jstar = min(sh->jstar, M - 1);  // M == 0 -> -1: nothing is split
            ctot = jstar >= 0 ? (int)(t5[jstar] & 0xffff) + (int)(t4[jstar] & 0xffff) : 0;
            // processed flag + creation base per node
            for (int p = tid; p < size; p += QT_THREADS) {
                const uint32_t r = t3[p];
                const bool proc = r != 0xffffffffu && (int)r <= jstar;
                t1[p] = proc ? (t5[r] & 0xffff) : 0;  // E[p]
                t0[p] = proc ? 0 : 1;                 // survivor
                meta[p] = (meta[p] & 0xffffu) | ((uint32_t)proc << 16);
            }
            __syncthreads();
            nmtot = (int)qt_block_scan<QT_THREADS>(t0, t2, size, sh);
        }
        // ---- D: build the next list (push_front order: child with creation rank r sits at ctot-1-r)
        for (int p = tid; p < size; p += QT_THREADS) {
            if ((meta[p] >> 16) & 1) {
                int r = (int)(t1[p] & 0xffff);
                for (int q = 0; q < 4; ++q) {
                    const uint32_t c = cc[4 * p + q];
                    if (c > 0) {
                        const int pos = ctot - 1 - r;
                        uint32_t c0, c1;
                        qt_child_box(box0[p], box1[p], q, c0, c1);
                        nbox0[pos] = c0; nbox1[pos] = c1; ncnt[pos] = c;
                        nmeta[pos] = (uint32_t)r | ((uint32_t)(c > 1) << 16);
                        newpos[4 * p + q] = (uint16_t)pos;
                        ++r;
                    }
                }
            } else {
                const int pos = ctot + (int)t2[p];
                nbox0[pos] = box0[p]; nbox1[pos] = box1[p]; ncnt[pos] = cnt[p];
                nmeta[pos] = 0;
                newpos[4 * p] = (uint16_t)pos;
            }
        }
        __syncthreads();
        // ---- E: keys follow their node
        const int new_size = ctot + nmtot;
        if (keys_in_reg) {
            // the quadrant is stage B's (0 for a node that did not count); a careful pass split only the nodes before the cut,
            // and stage C rewrote F to say which
#pragma unroll
            for (int j = 0; j < QT_KPT; ++j) {
                const int p = rnode[j] & 0xffff;
                int q = (rnode[j] >> 16) & 3;
                if (careful && !((meta[p] >> 16) & 1)) q = 0;
                rnode[j] = tid + j * QT_THREADS < K ? (uint32_t)newpos[4 * p + q] : 0u;
            }
        } else
        for (int k = tid; k < K; k += QT_THREADS) {
            const int p = knode[k];
            const int q = ((meta[p] >> 16) & 1) ? qt_quadrant(QT_KPOS(k), box0[p], box1[p]) : 0;
            knode[k] = (uint16_t)newpos[4 * p + q];
        }
        // stage E does not read the quadrant counters: zero them for the next pass here instead of in a stage of their own
        for (int p = tid; p < new_size; p += QT_THREADS) *(uint4 *)(cc + 4 * p) = make_uint4(0, 0, 0, 0);
        __syncthreads();
        { uint32_t *t;
          t = box0; box0 = nbox0; nbox0 = t;  t = box1; box1 = nbox1; nbox1 = t;
          t = cnt; cnt = ncnt; ncnt = t;      t = meta; meta = nmeta; nmeta = t; }
        // ---- termination (:1260-1283, :1363-1372)
        const bool done = new_size >= N || new_size == size;
        if (!careful && new_size + 3 * nexp_total > N) careful = true;
        size = new_size;   // every thread holds ctot + nmtot: the list size needs no LDS round trip
        if (done) break;
    }
    // ---- selection: best response, first in emission order
    for (int p = tid; p < size; p += QT_THREADS) best[p] = 0ull;
    __syncthreads();
    if (keys_in_reg) {
        uint32_t cy[QT_KPT];
#pragma unroll
        for (int j = 0; j < QT_KPT; ++j) { const int k = tid + j * QT_THREADS; cy[j] = k < K ? cand[k].y : 0u; }
#pragma unroll
        for (int j = 0; j < QT_KPT; ++j)
            if (tid + j * QT_THREADS < K) {
                const uint32_t cx = rpos[j];
                const unsigned long long key = ((unsigned long long)(((cx >> 24) << 24) | (0xffffffu - (cy[j] & 0xffffffu))) << 32) | cx;
                atomicMax(&best[rnode[j]], key);
            }
    } else
    for (int k = tid; k < K; k += QT_THREADS) {
        const uint2 c = cand[k];
        const unsigned long long key = ((unsigned long long)(((c.x >> 24) << 24) | (0xffffffu - (c.y & 0xffffffu))) << 32) | c.x;
        atomicMax(&best[knode[k]], key);
    }
    __syncthreads();
    const int nout = min(size, L.kp_cap);
    if (size > L.kp_cap && tid == 0) atomicMax(&status[f], (int)ORBX_CAPACITY);
    uint32_t *out = lvl_kp + (long long)f * g.kp_total + L.kp_begin;
    for (int p = tid; p < nout; p += QT_THREADS) out[p] = (uint32_t)best[p];
    if (tid == 0) lvl_count[f * g.nlevels + level] = nout;
}

template <int QT_THREADS>
__global__ __launch_bounds__(QT_THREADS, QT_THREADS == 256 ? 8 : QT_THREADS == 512 ? 6 : 4) void k_quadtree(DGeom g, const uint2 *__restrict__ dense_all,
                                                        const int *__restrict__ cand_count,
                                                        uint32_t *__restrict__ lvl_kp, int *__restrict__ lvl_count,
                                                        int *__restrict__ status, uint16_t *__restrict__ knode_glob,
                                                        int ncap, int lds_keys, int reg_keys, int level_begin) {
    const int level = level_begin + blockIdx.y, f = blockIdx.x;
    const int K = min(cand_count[f * g.nlevels + level], g.lv[level].cand_cap);
    if (K <= reg_keys * QT_THREADS)   // workgroup-uniform
        qt_workgroup<QT_THREADS, true>(g, dense_all, cand_count, lvl_kp, lvl_count, status, knode_glob, ncap, lds_keys, level_begin);
    else
        qt_workgroup<QT_THREADS, false>(g, dense_all, cand_count, lvl_kp, lvl_count, status, knode_glob, ncap, lds_keys, level_begin);
}

// ------------------------------------------------------------------------------------------------
// K4: IC_Angle (reference src/ORBextractor.cc:104-161) is fused into k_describe (K6): the orientation disc lies
// inside the LDS patch that kernel stages anyway.  Only the slot -> (level, index) helper remains here.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void orbx_slot_to_level(const DGeom &g, int slot, int &level, int &idx) {
    level = 0;
#pragma unroll
    for (int l = 1; l < ORBX_MAX_LEVELS; ++l)
        if (l < g.nlevels && slot >= g.lv[l].kp_begin) level = l;
    idx = slot - g.lv[level].kp_begin;
}

// ------------------------------------------------------------------------------------------------
// K5: GaussianBlur 7x7 sigma 2 (reference :2039-2047; OpenCV 3.2 fixed-point path, SURVEY App. B.4 +
// SSE2 column path: columns x < (w & ~3) accumulate in float with round-to-nearest-even, the last
// (w & 3) columns use the integer (s + 2^15) >> 16 tail).  Tile 64x16 per 256-thread block, staged in LDS.
// ------------------------------------------------------------------------------------------------
#define BL_TW 128
#define BL_TH 32
#define BL_SD ((BL_TW + 8) / 4)  // staged dwords per row: pixels [X0-4, X0+TW+4)
#define BL_ROWS (BL_TH + 6)
__global__ __launch_bounds__(256) void k_blur(DGeom g, const uint8_t *__restrict__ pyr, uint8_t *__restrict__ blur) {
    __shared__ uint32_t s_src[BL_ROWS * BL_SD];
    __shared__ __attribute__((aligned(8))) uint16_t s_h[BL_ROWS * BL_TW];
    const int tid = threadIdx.x, f = blockIdx.y;
    int level = 0;
    for (int l = 0; l < g.nlevels; ++l)
        if ((int)blockIdx.x >= g.lv[l].blur_tile_begin) level = l;
    const DLevel &L = g.lv[level];
    const int t = blockIdx.x - L.blur_tile_begin;
    const int ty = t / L.blur_tx, tx = t - ty * L.blur_tx;
    const int X0 = tx * BL_TW, Y0 = ty * BL_TH;
    const uint8_t *img = pyr + (long long)f * g.pyr_bytes + L.off;
    // ---- stage (TH+6) rows of (TW+8) pixels as aligned dwords; reflect-101 only on tiles touching the image edge
    for (int i = tid; i < BL_ROWS * BL_SD; i += 256) {
        const int r = i / BL_SD, d = i - r * BL_SD;
        const int sy = orbx_reflect101(Y0 + r - 3, L.ph);
        const int x = X0 - 4 + 4 * d;
        const uint8_t *row = img + (long long)sy * L.pitch;
        uint32_t v;
        if (x >= 0 && x + 3 < L.pw) {
            v = *(const uint32_t *)(row + x);
        } else {
            v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v |= (uint32_t)row[orbx_reflect101(x + k, L.pw)] << (8 * k);
        }
        s_src[i] = v;
    }
    __syncthreads();
    // ---- row pass: kernel {18,34,49,55,49,34,18} (float Gaussian * 256, rounded; sums to 257); 4 pixels per item
    for (int i = tid; i < BL_ROWS * (BL_TW / 4); i += 256) {
        const int r = i >> 5, q = i & 31;
        const uint32_t *w = s_src + r * BL_SD + q;
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
        int b[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b[k] = (w0 >> (8 * k)) & 0xff; b[4 + k] = (w1 >> (8 * k)) & 0xff; b[8 + k] = (w2 >> (8 * k)) & 0xff;
        }
        uint32_t h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            h[j] = 18 * (b[j + 1] + b[j + 7]) + 34 * (b[j + 2] + b[j + 6]) + 49 * (b[j + 3] + b[j + 5]) + 55 * b[j + 4];
        uint2 o;
        o.x = h[0] | (h[1] << 16);  // each <= 255 * 257 = 65535
        o.y = h[2] | (h[3] << 16);
        *(uint2 *)(s_h + r * BL_TW + 4 * q) = o;
    }
    __syncthreads();
    // ---- column pass: thread = 4 columns x 4 rows (10 staged rows), one dword store per output row
    const int cg = tid & 31, rg = tid >> 5;
    const int X = X0 + 4 * cg;
    if (X >= L.pw) return;
    // the SSE2 column path covers the columns x < (w & ~3) of the image GaussianBlur is given: the padded level (fork) or the
    // clone of the un-padded view (upstream: columns org .. org + sw - 1 here; its reflect-101 border is the level's own)
    const int wv = L.org + ((L.pw - 2 * L.org) & ~3);
    const float k0 = 55.f / 65536.f, k1 = 49.f / 65536.f, k2 = 34.f / 65536.f, k3 = 18.f / 65536.f;
    int hh[10][4];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint2 v = *(const uint2 *)(s_h + (rg * 4 + r) * BL_TW + 4 * cg);
        hh[r][0] = v.x & 0xffff; hh[r][1] = v.x >> 16; hh[r][2] = v.y & 0xffff; hh[r][3] = v.y >> 16;
    }
    uint8_t *out = blur + (long long)f * g.pyr_bytes + L.off;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int Y = Y0 + rg * 4 + j;
        if (Y >= L.ph) break;
        uint32_t outv = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r0 = hh[j + 3][i], r1 = hh[j + 2][i] + hh[j + 4][i], r2 = hh[j + 1][i] + hh[j + 5][i],
                      r3 = hh[j][i] + hh[j + 6][i];
            int o;
            if (X + i < wv) {
                float s0 = (float)r0 * k0 + 0.f;
                s0 = s0 + (float)r1 * k1;
                s0 = s0 + (float)r2 * k2;
                s0 = s0 + (float)r3 * k3;
                o = (int)__builtin_rintf(s0);
            } else {
                o = (55 * r0 + 49 * r1 + 34 * r2 + 18 * r3 + (1 << 15)) >> 16;
            }
            o = min(max(o, 0), 255);
            outv |= (uint32_t)o << (8 * i);
        }
        *(uint32_t *)(out + (long long)Y * L.pitch + X) = outv;
    }
}

// ------------------------------------------------------------------------------------------------
// K6: steered BRIEF-256 + keypoint assembly (reference computeOrbDescriptor :177-254, operator() :2049-2082).
// One wave per keypoint slot; 4 rounds x 64 lanes, one test pair per lane; __ballot packs 64 descriptor
// bits per round in the reference's bit order (bit i of byte j = pair 8j+i  ==  little-endian u64 words).
// ------------------------------------------------------------------------------------------------
// pattern rearranged per lane: entry l holds, for round r = 0..3, the pair r*64 + l as (x1, y1, x2, y2) int8
__constant__ int4 c_pattern_lane[64];
// IC_Angle weights (orbx_upload_pattern): lane = (disc row v + 15) * 2 + half; per lane the 5 aligned dwords of the LDS patch
// row it covers, as byte weights for v_dot4_u32_u8: [0..4] = u + 16 inside the disc (|u| <= umax[|v|]) else 0, [5..9] = 1
// inside the disc else 0.  m10 = sum(u * I) = dot(I, u + 16) - 16 * dot(I, 1), m01 = v * dot(I, 1): exact integers.
__constant__ uint32_t c_orient_w[64][12];
// B operands of the row pass on the matrix pipe: the banded 7-tap kernel, output column tile j of 16:
// entry [j][lane][.] = the 16 bytes B[k = 16 (lane >> 4) + s][n = lane & 15] = K7[k - (16 j + n)] (0 outside the band)
__constant__ uint32_t c_blur_b[3][64][4];

// The 7x7 Gaussian (reference :2039-2047) is fused in: only a 43x43 neighbourhood of each keypoint is ever sampled
// (|tap| <= 18, +3 px filter support), so each wave stages that patch of the UN-blurred level in LDS, runs the
// fixed-point row pass over it (4 pixels per item, as k_blur does) and evaluates the column pass only at the 512 tap
// positions.  The blurred image is never written: 2P bytes of HBM traffic per frame disappear.  Arithmetic is the
// same as k_blur's (8-bit kernel, float column path for x < (w & ~3), integer tail), so descriptors are unchanged.
#define DS_R 21                 // patch radius: 18 (taps) + 3 (filter support)
#define DS_W (2 * DS_R + 1)     // 43
#define DS_PP 44                // LDS patch pitch in bytes (11 dwords; rows start dword-aligned in LDS)
// The Gaussian's first pass is the ROW pass on the matrix pipe, which this kernel leaves idle while its vector pipe is the
// busiest port: H = (P - 128) x B + 128 * 257 with P the patch rows as int8 (x ^ 0x80), B the banded kernel (c_blur_b), as nine
// v_mfma_i32_16x16x64_i8 (3 row tiles x 3 column tiles, K = 64 patch columns at once), exact in int32.  The accumulator layout
// hands every lane FOUR CONSECUTIVE ROWS of one column, so the results are stored transposed for free -- HT[c][r], packed to u16
// pairs by one v_perm_b32 each, one ds_write_b64 per tile -- and the seven values a tap needs (vertical neighbours) are
// contiguous: 14 bytes inside one dword-aligned 16-byte window, folded by four v_dot2_u32_u16 against weights chosen by the
// parity of the tap's row (orbx_ds_tap).  The total I = sum_ij k_i k_j p[y+j][x+i] is one exact integer whichever pass runs
// first (every partial sum <= 255 * 257 = 65535), so the result is the same bit for bit.  The tap reads are what the LDS pipe
// of this kernel is busy with.  ~45 vector instructions for the pass instead of ~150.
// (The row pass on the vector pipe with seven ds_read_u16 per tap at an 80-byte stride, and the column pass over the whole
// patch in front of horizontal windows, came before this form: DESIGN.md, "the Gaussian's row pass on the matrix pipe"; the
// parent of this commit has the code.)
#define DS_VC 44                // pitch of HT in u16: the rows r of one column c (43 patch rows)
#define DS_VR 40                // columns c of HT the buffer holds (37 needed: taps -18..18)
#ifndef DS_WPB
#define DS_WPB 1   // waves (= keypoints) per block.  Nothing is shared between the waves of a block; one-wave blocks let the
                   // dispatcher place every wave as soon as any SIMD has room: 282 us against 299 (4 waves) and 372 (8)
#endif
// (Two or four consecutive keypoints per wave through the same LDS buffers, without prefetch, measured 314 / 319 us against
// 282 us in round 2: the kernel is not bound by the launch rate of its one-wave workgroups.)
// (Round 2 also rebuilt the column pass around the LDS counters -- the LDS pipe is active 87 % of this kernel, 60 % of that
// bank conflicts of the 56 ds_read_u16 per lane at the rotated tap positions: row-pass output stored TRANSPOSED in two
// copies (A[c][r] = h[r][c], B[c][r] = h[r + 2][c]) so that a tap's seven vertical neighbours always sit in one 8-byte
// aligned 16-byte window, fetched by ONE ds_read2_b64 and folded by v_alignbit + four v_dot2_u32_u16; the patch aliased
// into copy B.  Bit-exact, 8 instead of 56 LDS reads per lane -- and 324 us against 281 us: the transposed stores and the
// window addressing cost ~95 more vector instructions per keypoint, and with both pipes near saturation it is the vector
// pipe that sets the time.  Not kept.)
#ifndef DS_WPS
#define DS_WPS 7   // waves per SIMD the register allocation must allow (LDS admits 7 blocks of 4 waves per CU)
#endif
// (Several keypoints per wave with register prefetch of the next patch was measured: 430-440 us at the 4-5 waves per
// SIMD its registers allow against 375 us for one keypoint per wave -- every phase of this kernel is a dependent chain of
// LDS round trips, and resident waves are what hides them.)
// The length of one wave's dependent chain (profiles/describe_chain.md):
// Waves are indexed by the SLOT of the per-frame level-keypoint table, not by output position.  The level of a slot
//   follows from the kp_begin values (kernel arguments) alone, so the level's table entry, the eight counts and the slot's
//   position word are requested together, in front of one wait: kernel arguments, {level entry, counts, position}, patch -- three
//   memory round trips in front of the first LDS write where an output-indexed wave has eight.  A slot beyond its level's count
//   is a dead wave; the output position is the sum of the counts below the level + the index in the level.  Slot order is
//   level-major like the output order, so the order of the workgroups of a frame on its XCD is the same.
// The constant tables (pattern, c_orient_w, c_blur_b) are requested right behind the patch loads, before the first LDS write,
//   not in front of their first use.
// The taps run one after the other: batches of 2 / 4 / 8 (all addresses, all LDS reads, then independent dot-product chains)
//   measured slower or equal.  The pattern coordinates are 16 int8 -> float conversions per lane: as a float table, four
//   16-byte loads per lane in place of one cost more.  (Both in profiles/describe_chain.md; the parent of this commit has the code.)
// FPM (fp_mode) is a template constant: as a run-time value it costs a scalar branch and both code paths in each of the 8 taps
typedef const __attribute__((address_space(3))) uint16_t *orbx_lds_u16p;
typedef const __attribute__((address_space(3))) uint32_t *orbx_lds_u32p;
// I = sum_i k_i HT[c][r + i], i = 0..6, for the u16 element at LDS byte address `adr`: the 8 elements of the dword-aligned
// 16-byte window around them, against the weights shifted by the parity of r; I < 2^24.01.
__device__ __forceinline__ uint32_t orbx_ds_tap(uint32_t adr) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const orbx_lds_u32p wp = (orbx_lds_u32p)(uintptr_t)(adr & ~3u);
    const uint32_t d[4] = {wp[0], wp[1], wp[2], wp[3]};
    const bool odd = (adr & 2u) != 0;
    const uint32_t w[4] = {odd ? (18u << 16) : (18u | (34u << 16)), odd ? (34u | (49u << 16)) : (49u | (55u << 16)),
                           odd ? (55u | (49u << 16)) : (49u | (34u << 16)), odd ? (34u | (18u << 16)) : 18u};
    uint32_t I = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) I = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, d[i]), __builtin_bit_cast(u16x2, w[i]), I, false);
    return I;
}
// INPLACE: level-0 keypoints stage their patch from the caller's grey image (`raw`), which holds no border: interior
// keypoints run the slab path's code on it; a patch that leaves the raw image (about 15 % of the level-0 keypoints: the 19-pixel
// border of the padded level is gone) takes its rows through the reflection, loads one 48-byte window per row that is clamped
// into the row, lays it into LDS displaced by whole dwords + the usual funnel shift, and then mirrors the ring columns from
// the LDS row itself.  Address arithmetic: orbx_inplace.h.
template <int FPM, bool INPLACE>
__global__ __launch_bounds__(64 * DS_WPB, DS_WPS) void k_describe(DGeom g, const uint8_t *__restrict__ pyr,
                                                  const uint32_t *__restrict__ lvl_kp,
                                                  const int *__restrict__ lvl_count,
                                                  float *__restrict__ lvl_angle, orbx_keypoint *__restrict__ kps,
                                                  uint8_t *__restrict__ desc, int *__restrict__ counts,
                                                  int *__restrict__ status, int cap, int dbg_stop, int nframes, OrbxRaw0 raw) {
    // dbg_stop (ORBX_DESC_STOP, phase-timing builds only, -DORBX_TIMING_KNOBS): 1 = after staging, 2 = after orientation,
    // 3 = after the row pass.  The shipped library pins it to 0.
#ifndef ORBX_TIMING_KNOBS
    dbg_stop = 0;
#endif
    // HT OVER the patch: the row pass holds every patch row it needs in registers before its first store (a wave's LDS
    // instructions execute in order, and one wave owns the buffers), and nothing reads the patch afterwards -- 3.5 KB of LDS per
    // wave instead of 5.4
    __shared__ __attribute__((aligned(16))) uint16_t s_h[DS_WPB][DS_VR * DS_VC];
    // one wave per keypoint slot.  The wave index is wave-uniform (which the compiler cannot see): with it scalar, the level search and the position
    // load run on the scalar unit.
    const int lane = threadIdx.x & 63, wv_id = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // Workgroup order (x fastest): frame mod 8, then keypoint, then frame / 8.  Workgroups are dealt round-robin over the 8
    // XCDs, so XCD x works through the keypoints of frame 8k + x one after the other with that frame's 1.2 MB pyramid in its
    // own 4 MB L2, and the chip holds 8 frames at a time.  (With the frame as the fastest index -- the order of the first
    // version -- every frame of the batch has a few keypoints in flight at once: at 1024 frames per launch no cache holds that,
    // and every patch came from HBM, 3.1 MB per frame.)
    // every kernel argument the path to the first patch load reads, requested in front of ONE wait (left alone, each is loaded
    // in front of its first use: one round trip per basic block of the prologue)
    // (the empty asm only fixes the point by which all of them have arrived.  Not volatile, and with results that are used: a
    // volatile asm counts as a store to memory, behind which no load through a pointer argument is a scalar load any more.)
    int kbv[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) kbv[l] = g.lv[l].kp_begin;
    asm("" : "+s"(nframes), "+s"(cap), "+s"(kbv[0]), "+s"(kbv[1]), "+s"(kbv[2]), "+s"(kbv[3]), "+s"(kbv[4]), "+s"(kbv[5]), "+s"(kbv[6]), "+s"(kbv[7])
           : "s"(g.nlevels), "s"(g.kp_total), "s"(g.pyr_bytes), "s"(lvl_kp), "s"(lvl_count), "s"(pyr));
    const int f = blockIdx.y * 8 + (blockIdx.x & 7);
    const int wi = (blockIdx.x >> 3) * DS_WPB + wv_id;
    if (f >= nframes) return;
    const int *lc = lvl_count + f * g.nlevels;
    int total = 0, level = 0;
    // wave = slot.  (First round trip: the kernel arguments, pinned at the top of the kernel.)
    const int slot = wi;
    if (DS_WPB > 1 && slot >= g.kp_total) return;
    const bool all8 = g.nlevels == 8;   // every ORB-SLAM2 configuration
    int kb = kbv[0];
    if (all8) {
#pragma unroll
        for (int l = 1; l < 8; ++l)
            if (slot >= kbv[l]) { level = l; kb = kbv[l]; }
    } else {
#pragma unroll
        for (int l = 1; l < ORBX_MAX_LEVELS; ++l)
            if (l < g.nlevels && slot >= g.lv[l].kp_begin) { level = l; kb = g.lv[l].kp_begin; }
    }
    // Second round trip: the level's table entry, the slot's position word and the counts, all addressable now.  (The position
    // word of a dead slot is read and dropped: slot < kp_total lies inside the frame's table whatever the counts are.)
    uint32_t pos = lvl_kp[(long long)f * g.kp_total + slot];
    struct { int pw, ph, pitch, org; long long off; float scale, size; } L =
        {g.lv[level].pw, g.lv[level].ph, g.lv[level].pitch, g.lv[level].org, g.lv[level].off, g.lv[level].scale, g.lv[level].size};
    int base = 0, mine = 0;
    if (all8) {
        int4 ca = *(const int4 *)lc, cb = *(const int4 *)(lc + 4);
        // one wait for the whole round trip: without the pin the compiler sinks each load to its first use, behind the exits below
        asm("" : "+s"(pos), "+s"(L.pw), "+s"(L.ph), "+s"(L.pitch), "+s"(L.org), "+s"(L.off), "+s"(L.scale), "+s"(L.size),
                 "+s"(ca.x), "+s"(ca.y), "+s"(ca.z), "+s"(ca.w), "+s"(cb.x), "+s"(cb.y), "+s"(cb.z), "+s"(cb.w));
        const int cnt[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            if (l < level) base += cnt[l];
            if (l == level) mine = cnt[l];
            total += cnt[l];
        }
    } else {
#pragma unroll
        for (int l = 0; l < ORBX_MAX_LEVELS; ++l) {
            if (l < g.nlevels) {
                const int c = lc[l];
                if (l < level) base += c;
                if (l == level) mine = c;
                total += c;
            }
        }
    }
    const int oi = base + (slot - kb);   // dense output position (level-major order of operator(), :2066-2082)
    if (slot == 0 && lane == 0) {        // slot 0 exists in every frame, live or not
        counts[f] = min(total, cap);
        if (total > cap) atomicMax(&status[f], (int)ORBX_CAPACITY);
    }
    if (slot - kb >= mine || oi >= min(total, cap) || dbg_stop == 4) return;
    uint32_t *patch = (uint32_t *)s_h[wv_id];
    uint16_t *hrow = s_h[wv_id];
    // the constant tables, requested right behind the patch loads (the scheduling barrier keeps every patch load in front of
    // them: loads return in order, and the first LDS write waits for the patch alone)
    int4 pat;
    uint4 wa, wb, wc;
    uint4 b4[3];
#define DS_LOAD_EARLY() do {                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                                   \
        pat = c_pattern_lane[lane];                                                                                          \
        wa = *(const uint4 *)&c_orient_w[lane][0]; wb = *(const uint4 *)&c_orient_w[lane][4]; wc = *(const uint4 *)&c_orient_w[lane][8]; \
        _Pragma("unroll") for (int j = 0; j < 3; ++j) b4[j] = *(const uint4 *)&c_blur_b[j][lane][0];                         \
    } while (0)
    const int x = (int)(pos & 0xfff) + (ORBX_EDGE - 3), y = (int)((pos >> 12) & 0xfff) + (ORBX_EDGE - 3);
    const bool ip0 = INPLACE && level == 0;   // wave-uniform
    const uint8_t *img = ip0 ? raw.img + (long long)f * raw.frame_stride : pyr + (long long)f * g.pyr_bytes + L.off;
    const int spitch = ip0 ? raw.stride : L.pitch;
    // patch origin in the coordinates of the image the patch is staged from
    // (x, y are coordinates of mvImagePyramid[level]; that image starts at (L.org, L.org) of the slab's padded level)
    const int px0 = x - DS_R + (ip0 ? -ORBX_EDGE : L.org), py0 = y - DS_R + (ip0 ? -ORBX_EDGE : L.org);
    const int xa = px0 & ~3;
    const bool interior = ip0 ? orbx_ip_desc_interior(px0, py0, raw.W, raw.H)
                              : px0 >= 0 && py0 >= 0 && xa + 48 <= L.pitch && px0 + 2 * DS_R < L.pw && py0 + 2 * DS_R < L.ph;
    {
        // ---- stage the 43x43 patch (rows y-21.., columns x-21..): 12 ALIGNED dwords cover the 44 bytes of a patch
        // row; dword d of the LDS row = funnel shift of aligned dwords d, d+1.  A lane loads 3 aligned dwords (one
        // 12-byte load: a third of the load instructions of a dword per lane, the texture-address unit's rate is per
        // lane, not per byte) and takes the 4th from the lane above (one DPP move): 4 lanes per row, 16 rows per step,
        // every load in flight before the first LDS write.
        if (interior) {
            const int dq = lane & 3, rq = lane >> 2;
            const uint32_t shift = (uint32_t)(px0 & 3);
            const uint8_t *p0 = img + (__mul24(py0, spitch) + xa + 12 * dq);   // 32-bit offsets: no 64-bit multiplies
            orbx_uint3_u tv[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) tv[k] = *(const orbx_uint3_u *)(p0 + __mul24(min(16 * k + rq, DS_W - 1), spitch));
            DS_LOAD_EARLY();
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t nxt = orbx_lane_above(tv[k].x);
                const int r = 16 * k + rq;
                if (r < DS_W) {
                    uint32_t *d = patch + r * (DS_PP / 4) + 3 * dq;
                    d[0] = __builtin_amdgcn_alignbyte(tv[k].y, tv[k].x, shift);
                    d[1] = __builtin_amdgcn_alignbyte(tv[k].z, tv[k].y, shift);
                    if (dq < 3) d[2] = __builtin_amdgcn_alignbyte(nxt, tv[k].z, shift);   // dword 11 of a row does not exist
                }
            }
        } else if (ip0) {
            // patch columns c <-> raw columns px0 + c; window byte i <-> raw column ws + i <-> patch column i + (ws - px0).
            // LDS dword D of a row = window bytes [4 D + e, + 4) with e = px0 - ws (any sign): window dwords D + (e >> 2) and the
            // next one, funnel-shifted by e & 3.  Lane dq holds window dwords 3 dq .. 3 dq + 2 and takes the 4th from the lane above.
            const int dq = lane & 3, rq = lane >> 2;
            const int ws = orbx_ip_desc_ws(px0, raw.W);
            const int e = px0 - ws;
            const uint32_t shift = (uint32_t)(e & 3);
            const int dd = e >> 2;                                  // window dword of LDS dword 0 (floor)
            orbx_uint3_u tv[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                tv[k] = *(const orbx_uint3_u *)(img + orbx_ip_row_off(orbx_ip_map(py0 + ORBX_EDGE + min(16 * k + rq, DS_W - 1), raw.H), raw.stride, ws + 12 * dq));
            DS_LOAD_EARLY();
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t nxt = orbx_lane_above(tv[k].x);
                const int r = 16 * k + rq;
                if (r < DS_W) {
                    uint32_t *d = patch + r * (DS_PP / 4);
                    const int D = 3 * dq - dd;                      // LDS dword of this lane's first funnel
                    // (the last window dword of a row has no successor: its funnel carries bytes of the next row's lane in
                    // its top `shift` bytes, which are ring columns beyond W whenever that dword is stored)
                    const uint32_t f0 = __builtin_amdgcn_alignbyte(tv[k].y, tv[k].x, shift), f1 = __builtin_amdgcn_alignbyte(tv[k].z, tv[k].y, shift),
                                   f2 = __builtin_amdgcn_alignbyte(nxt, tv[k].z, shift);
                    if (D >= 0 && D < DS_PP / 4) d[D] = f0;
                    if (D + 1 >= 0 && D + 1 < DS_PP / 4) d[D + 1] = f1;
                    if (D + 2 >= 0 && D + 2 < DS_PP / 4) d[D + 2] = f2;
                    // the dword in front of window dword 0 (left edge: its top bytes are raw columns 0 ..)
                    if (dq == 0 && D - 1 >= 0 && D - 1 < DS_PP / 4) d[D - 1] = __builtin_amdgcn_alignbyte(tv[k].x, 0u, shift);
                }
            }
            // ring columns (raw column < 0 or >= W), one per step, lane = patch row: mirrored from the row's own real columns
            // (source position 0..43 of the 44 staged bytes); the one position that can fall in front of the row
            // (right edge, 37 <= c) is read from the image
            const int c_end_l = px0 < 0 ? min(-px0, DS_W) : 0, c_beg_r = max(raw.W - px0, 0);
            if (c_end_l > 0 || c_beg_r < DS_W) {
                orbx_wave_sync();
                uint8_t *pb = (uint8_t *)patch + min(lane, DS_W - 1) * DS_PP;
                const uint8_t *grow = img + orbx_ip_row_off(orbx_ip_map(py0 + ORBX_EDGE + min(lane, DS_W - 1), raw.H), raw.stride, 0);
                for (int c = 0; c < DS_W; ++c) {
                    if (c >= c_end_l && c < c_beg_r) { c = c_beg_r - 1; continue; }
                    const int j = orbx_ip_map(px0 + ORBX_EDGE + c, raw.W);   // wave-uniform
                    const int sp = j - px0;
                    const uint8_t v = (sp >= 0 && sp < DS_PP) ? pb[sp] : grow[j];
                    if (lane < DS_W) pb[c] = v;
                }
            }
        } else {
            // image edge: reflect-101 of the padded level, byte by byte
            uint8_t *pb = (uint8_t *)patch;
            DS_LOAD_EARLY();
            for (int i = lane; i < DS_W * DS_W; i += 64) {
                const int r = i / DS_W, c = i - r * DS_W;
                const int sy = orbx_reflect101(py0 + r, L.ph), sx = orbx_reflect101(px0 + c, L.pw);
                pb[r * DS_PP + c] = img[(long long)sy * L.pitch + sx];   // (never the in-place image: !ip0 here)
            }
        }
        orbx_wave_sync();
        if (dbg_stop == 1) return;
        // ---- orientation (IC_Angle, reference src/ORBextractor.cc:104-161) from the staged UN-blurred patch: lanes 0-31
        // take the row +v, lanes 32-63 the row -v; integer moments reduced across the wave; fastAtan2 on every lane
        float angle_deg;
        {
            // lane = (row, half): 5 aligned dwords of patch row 21 + v, two v_dot4_u32_u8 each against the constant weights
            const int row = lane >> 1, half = lane & 1;                 // row = v + 15 (lanes 62, 63 carry zero weights)
            const uint32_t *pr = patch + min(row + (DS_R - ORBX_HALF_PATCH), DS_W - 1) * (DS_PP / 4) + 1 + 5 * half;
            const uint32_t p0 = pr[0], p1 = pr[1], p2 = pr[2], p3 = pr[3], p4 = pr[4];
            uint32_t A = __builtin_amdgcn_udot4(p0, wa.x, 0u, false), S = __builtin_amdgcn_udot4(p0, wb.y, 0u, false);
            A = __builtin_amdgcn_udot4(p1, wa.y, A, false); S = __builtin_amdgcn_udot4(p1, wb.z, S, false);
            A = __builtin_amdgcn_udot4(p2, wa.z, A, false); S = __builtin_amdgcn_udot4(p2, wb.w, S, false);
            A = __builtin_amdgcn_udot4(p3, wa.w, A, false); S = __builtin_amdgcn_udot4(p3, wc.x, S, false);
            A = __builtin_amdgcn_udot4(p4, wb.x, A, false); S = __builtin_amdgcn_udot4(p4, wc.y, S, false);
            int m10 = (int)A - 16 * (int)S;
            int m01 = __mul24(row - ORBX_HALF_PATCH, (int)S);
            m10 = orbx_wave_sum(m10);
            m01 = orbx_wave_sum(m01);
            angle_deg = orbx_fast_atan2((float)m01, (float)m10);
            if (lane == 0) lvl_angle[(long long)f * g.kp_total + slot] = angle_deg;
        }
        if (dbg_stop == 2) return;
        // ---- row pass: h[r][c] for patch columns c+3 (c = 0..36 used), on the matrix pipe, stored transposed (HT[c][r]) over the patch
        {
            typedef int i32x4 __attribute__((ext_vector_type(4)));
            const int m = lane & 15, gq = lane >> 4;
            i32x4 A[3], Bm[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) {   // A[t]: patch row 16 t + m, bytes 16 gq .. + 15 (rows >= 43 / bytes >= 43: don't-care, zero weights or unused rows)
                const uint32_t *ap = patch + (16 * t + m) * (DS_PP / 4) + 4 * gq;
                A[t][0] = (int)(ap[0] ^ 0x80808080u); A[t][1] = (int)(ap[1] ^ 0x80808080u);
                A[t][2] = (int)(ap[2] ^ 0x80808080u); A[t][3] = (int)(ap[3] ^ 0x80808080u);
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                Bm[j][0] = (int)b4[j].x; Bm[j][1] = (int)b4[j].y; Bm[j][2] = (int)b4[j].z; Bm[j][3] = (int)b4[j].w;
            }
            const i32x4 c0 = {128 * 257, 128 * 257, 128 * 257, 128 * 257};
            uint32_t *vo = (uint32_t *)hrow + m * (DS_VC / 2) + 2 * gq;   // HT[c = 16 j + m][r = 16 t + 4 gq ..]: u16 index c * 44 + r
#pragma unroll
            for (int j = 0; j < 3; ++j) {
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const i32x4 acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], Bm[j], c0, 0, 0, 0);
                    // columns c < 37 and rows r < 44 exist in HT
                    if ((j < 2 || m < DS_W - 6 - 32) && (t < 2 || gq < 3))
                        // every accumulator is a sum of bytes x the 8-bit kernel (<= 255 * 257, whatever bytes the don't-care rows
                        // hold): its two low bytes are the whole value
                        *(uint2 *)(vo + (16 * j) * (DS_VC / 2) + 8 * t) =
                            make_uint2(__builtin_amdgcn_perm((uint32_t)acc[1], (uint32_t)acc[0], 0x05040100u),
                                       __builtin_amdgcn_perm((uint32_t)acc[3], (uint32_t)acc[2], 0x05040100u));
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (dbg_stop == 3) return;
        // ---- taps
        const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
        const float angle = angle_deg * factorPI;
                const OrbxSinCos sc = orbx_sincosf_pinned(angle);
        const float a = sc.c, b = sc.s;
        // Column pass at the tap position.  OpenCV's SSE2 column filter accumulates ((r0*k0 + r1*k1) + r2*k2) + r3*k3 in
        // float with k = {55,49,34,18}/65536 and rounds to nearest-even for the columns x < (w & ~3); the last w & 3
        // columns take its integer tail (I + 2^15) >> 16.  Every float product and every partial sum below 2^24 units of
        // 2^-16 is exact, and a total >= 2^24 saturates to 255 either way, so the float path IS round-half-even(I / 65536)
        // with I = 55 r0 + 49 r1 + 34 r2 + 18 r3: one integer formula serves both, the tail only changes the tie rule.
        const int wvec = (L.pw - 2 * L.org) & ~3;   // of the image GaussianBlur is given (fork: the padded level; upstream: the view)
        // tap t = 2 r + s2: point s2 of the lane's pair of round r
        const int pw4[4] = {pat.x, pat.y, pat.z, pat.w};
#define DS_PX(t) ((float)(signed char)((pw4[(t) >> 1] >> (16 * ((t) & 1))) & 0xff))
#define DS_PY(t) ((float)(signed char)((pw4[(t) >> 1] >> (16 * ((t) & 1) + 8)) & 0xff))
        unsigned long long words[4];
        if (x + (DS_R - 3) < wvec) {
            // No tap of this keypoint reaches the tail columns (all but keypoints within 18 px of the right edge): the
            // float form of round-half-even is the shortest.  cvRound of the rotated coordinates = adding 1.5 * 2^23
            // (round-to-nearest-even in the add, the integer lands in the low mantissa bits); the 24-bit multiply-add
            // takes those low bits as they are, the exponent bits of the column term cancel in the constant.
            const uint32_t cbias = (uint32_t)(2 * ((DS_R - 3) * DS_VC + (DS_R - 3))) - 0x400000u * (2u * DS_VC) - (0x4B400000u << 1);
            const uint32_t hbase = (uint32_t)(uintptr_t)(orbx_lds_u16p)hrow + cbias;
            float tv[8];
            float nb = -b;
            asm("" : "+v"(nb));   // a register of its own (the compiler would fold the negation back into every product)
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const float px = DS_PX(t), py = DS_PY(t);
                // fy = x*b + rn(y*a) (vfmadd132ss), fx = x*a - rn(y*b) (vfmsub132ss); -(y*b) = y*(-b) exactly, and a product by a
                // NEGATED REGISTER is a VOP3 encoding (half rate).  fx is formed behind the pin of the row address: where the
                // compiler's schedule of the eight taps wants it
                const float fy = FPM == ORBX_FP_GCC_FMA ? __builtin_fmaf(px, b, py * a) : px * b + py * a;
                const uint32_t uy = __float_as_uint(fy + 12582912.0f);
                // LDS byte address of HT[ix+18][iy+18]: the tap's window starts here (two instructions: v_lshl_add + v_mad_u32_u24)
                uint32_t ay = (uy << 1) + hbase;
                asm("" : "+v"(ay));
                const float fx = FPM == ORBX_FP_GCC_FMA ? __builtin_fmaf(px, a, py * nb) : px * a + py * nb;
                const uint32_t ux = __float_as_uint(fx + 12582912.0f);
                const uint32_t I = orbx_ds_tap(__umul24(ux, 2u * DS_VC) + ay);
                // I <= 2^24 converts exactly and I * 2^-16 is exact; above, the conversion's own rounding keeps it >= 256
                tv[t] = __builtin_fminf(__builtin_rintf((float)I * (1.f / 65536.f)), 255.f);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) words[r] = orbx_ballot(tv[2 * r] < tv[2 * r + 1]);
        } else {
            int tval[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const float px = DS_PX(t), py = DS_PY(t);
                float fy, fx;
                if (FPM == ORBX_FP_GCC_FMA) {
                    fy = __builtin_fmaf(px, b, py * a);
                    fx = __builtin_fmaf(px, a, -(py * b));
                } else {
                    fy = px * b + py * a;
                    fx = px * a - py * b;
                }
                const int iy = (int)__builtin_rintf(fy), ix = (int)__builtin_rintf(fx);
                // blurred pixel (x+ix, y+iy): column pass over h rows (iy+21-3 .. iy+21+3), h column ix+18
                const uint32_t I = orbx_ds_tap((uint32_t)(uintptr_t)(orbx_lds_u16p)hrow + 2u * (uint32_t)(__mul24(ix + DS_R - 3, DS_VC) + (iy + DS_R - 3)));
                const uint32_t tie = x + ix >= wvec ? 1u : ((I >> 16) & 1u);   // half-up in the tail, half-even elsewhere
                tval[t] = (int)min((I + 0x7fffu + tie) >> 16, 255u);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) words[r] = orbx_ballot(tval[2 * r] < tval[2 * r + 1]);
        }
        if (lane < 4) {
            unsigned long long w = lane == 0 ? words[0] : lane == 1 ? words[1] : lane == 2 ? words[2] : words[3];
            *(unsigned long long *)(desc + ((long long)f * cap + oi) * 32 + 8 * lane) = w;
        }
        if (lane == 0) {
            orbx_keypoint kp;
            float fx = (float)x, fy = (float)y;
            if (level != 0) { fx = fx * L.scale; fy = fy * L.scale; }
            kp.x = fx; kp.y = fy;
            kp.size = L.size;
            kp.angle = angle_deg;
            kp.response = (float)(pos >> 24);
            kp.octave = level;
            kp.class_id = -1;
            kps[(long long)f * cap + oi] = kp;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K7: brute-force Hamming best / second-best (DescriptorDistance src/ORBmatcher.cc:2073-2093 for every
// pair; bookkeeping of the search loops, e.g. :627-640) on the matrix cores.
//
// nq x nt x 256 bit operations per pair is GEMM-shaped and compute-bound (16 MB of descriptors against 65 G bit
// products per 256-frame step), so the distances come from v_mfma_i32_32x32x32_i8:
//     dist(q, t) = popc(q) + popc(t) - 2 * <q, t>           (<.,.> = dot product of the two bit vectors)
//   * A operand = 32 TRAIN descriptors of a tile, bit p of their 32 bytes expanded to bytes 0 / 64 (shift + and per
//     dword; K-step p = bit p of every byte: the K order is irrelevant as long as both operands use the same one);
//   * B operand = 32 QUERY descriptors, expanded ONCE per wave to bytes 0 / -128 and kept in registers (two query tiles
//     per wave: 64 VGPRs), so that every product is 0 or -8192 = -2 << 12;
//   * the accumulator of a tile is not cleared but LOADED with key(t) = (popc(t) + 256) << 12 | index-in-chunk from an
//     LDS table (the C layout puts 4 consecutive train rows in 4 consecutive registers: one ds_read_b128 each), so
//     eight MFMAs leave  key = (dist - popc(q) + 256) << 12 | index  in every accumulator register -- ordered like
//     (dist, index) for the lane's query -- and the bookkeeping is two instructions per distance: second =
//     med3(key, best, second), best = min(best, key).  min(key) is the best match with the lowest index on ties and the
//     second-smallest key carries the second-best distance counting duplicates, exactly the reference loops.
// Measured on 256 x 1000 x 1000 (tools/match_rate.py): 60 us; without the bookkeeping 48 us, without the expansion of the
// train tiles 56 us, MFMAs + loads alone 49 us (= 2.7 Pop/s: the matrix pipe at the clock the chip holds under this load).
// The same kernel on v_mfma_i32_16x16x64_i8 (four 16-column query tiles per wave, K step = two bit planes) is bit-exact
// and slower, 71 us: twice the operand traffic per product and rotates instead of shifts in the expansion.
// 174 -> 60-65 us per 256 x 1000 x 1000 against k_match_valu below (xor + popcount on the vector pipe), which north_star
// names as the form of this kernel ("no MFMA -- this is integer/bitwise work"): the premise does not hold for the matcher
// -- the result is the same integer, bit for bit -- so the MFMA kernel is the default and the vector-pipe kernel stays
// selectable (ORBX_MATCH_KERNEL=valu) and parity-tested, for A/B runs and for readers who want the path as specified.
// ------------------------------------------------------------------------------------------------
// (MT_SPLIT, the most ways the train set is split over blockIdx.y, and MT_QPW: orbx_launch.h, beside the launcher's rule)
#define MT_WAVES 4      // waves per block; they share the train key table
// Query column tiles (of 32) per wave, QT: the expanded train tile (A operand: 32 shift-and pairs) and its key registers serve QT
// MFMA chains.  QT = 2: 64 B-operand registers, three waves per SIMD without a spill (round 2 capped the registers for four
// and spilled 11 of them inside the MFMA loop).  QT = 4: a block walks its train tiles ONCE for 512 queries -- half the train
// loads, half the expansions and half the key-table reads per distance -- with 128 B-operand + 64 accumulator registers, two
// waves per SIMD; the launcher takes it when the launch still fills the chip that way.
#define MT_QPB(QT) (MT_WAVES * MT_QPW(QT))
#define MT_CHUNK 4096   // train descriptors per key table (12 index bits in the key)
typedef int mt_v4i __attribute__((ext_vector_type(4)));
typedef int mt_v16i __attribute__((ext_vector_type(16)));
__device__ __forceinline__ uint32_t mt_min2(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t mt_max2(uint32_t a, uint32_t b) { return a > b ? a : b; }
template <int QT>
__global__ __launch_bounds__(64 * MT_WAVES, QT == 2 ? 3 : 2) void k_match(const uint8_t *__restrict__ q, const int *__restrict__ nq,
                                                         long long q_stride, const uint8_t *__restrict__ t,
                                                         const int *__restrict__ nt, long long t_stride,
                                                         uint2 *__restrict__ partial, int *__restrict__ best_idx,
                                                         int *__restrict__ best_dist, int *__restrict__ second_dist,
                                                         int out_stride, int nsplit) {
    __shared__ __attribute__((aligned(16))) int s_tk[MT_CHUNK];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), pr = blockIdx.z, sp = blockIdx.y;
    const int NQ = min(nq[pr], out_stride), NT = min(nt[pr], 1 << 20);   // contract (orbx.h): counts beyond out_stride are ignored
    if ((int)blockIdx.x * MT_QPB(QT) >= NQ) return;
    const int r = lane & 31, h = lane >> 5;
    const uint8_t *qp = q + (long long)pr * q_stride;
    const uint8_t *tp = t + (long long)pr * t_stride;
    // this block's share of the train set, in whole tiles of 32
    const int per = ((NT + 31) / 32 + nsplit - 1) / nsplit * 32;
    const int j0 = min(NT, sp * per), j1 = min(NT, j0 + per);
    // ---- queries: lane (r, h) holds bytes 16h .. 16h+15 of query r of each tile, expanded bit plane by bit plane
    const int qw = blockIdx.x * MT_QPB(QT) + w * MT_QPW(QT);
    const bool wave_on = qw < NQ;
    mt_v4i bq[QT][8];
    int pq[QT];
#pragma unroll
    for (int c = 0; c < QT; ++c) {
        const int qi = qw + 32 * c + r;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (qi < NQ) v = *(const uint4 *)(qp + (long long)qi * 32 + 16 * h);
        pq[c] = __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
        pq[c] += __shfl_xor(pq[c], 32);
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            bq[c][p][0] = (int)((v.x << (7 - p)) & 0x80808080u);
            bq[c][p][1] = (int)((v.y << (7 - p)) & 0x80808080u);
            bq[c][p][2] = (int)((v.z << (7 - p)) & 0x80808080u);
            bq[c][p][3] = (int)((v.w << (7 - p)) & 0x80808080u);
        }
    }
    // running result over the chunks, in the output format dist << 20 | index
    uint32_t gbest[QT], gsecond[QT];
#pragma unroll
    for (int c = 0; c < QT; ++c) gbest[c] = gsecond[c] = 0xffffffffu;
    for (int c0 = j0; c0 < j1; c0 += MT_CHUNK) {
        const int c1 = min(j1, c0 + MT_CHUNK), n = c1 - c0, npad = (n + 31) & ~31;
        __syncthreads();   // the previous chunk's table is no longer read
        for (int i = threadIdx.x; i < npad; i += 64 * MT_WAVES) {
            int key = 0x7fffffff;   // rows past the end: never the minimum (their descriptor is read as zero below)
            if (i < n) {
                const uint4 a = *(const uint4 *)(tp + (long long)(c0 + i) * 32), b = *(const uint4 *)(tp + (long long)(c0 + i) * 32 + 16);
                const int pt = __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(b.x) + __popc(b.y) + __popc(b.z) + __popc(b.w);
                key = ((pt + 256) << 12) | i;
            }
            s_tk[i] = key;
        }
        __syncthreads();
        if (!wave_on) continue;
        int best[QT], second[QT];
#pragma unroll
        for (int c = 0; c < QT; ++c) best[c] = second[c] = 0x7fffffff;
        const uint8_t *trow = tp + (long long)(c0 + r) * 32 + 16 * h;
        uint4 ta = make_uint4(0, 0, 0, 0);
        if (r < n) ta = *(const uint4 *)trow;
        for (int jt = 0; jt < npad; jt += 32) {
            const uint4 tc = ta;
            // next tile's descriptors requested before this tile's MFMAs
            ta = make_uint4(0, 0, 0, 0);
            if (jt + 32 + r < n) ta = *(const uint4 *)(trow + (long long)(jt + 32) * 32);
            mt_v16i acc[QT];
            {
                const int4 *kp = (const int4 *)(s_tk + jt + 4 * h);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int4 k4 = kp[2 * g];   // rows 8g + 4h .. + 3 of the tile = registers 4g .. 4g+3
                    acc[0][4 * g] = k4.x; acc[0][4 * g + 1] = k4.y; acc[0][4 * g + 2] = k4.z; acc[0][4 * g + 3] = k4.w;
                }
#pragma unroll
                for (int c = 1; c < QT; ++c) acc[c] = acc[0];
            }
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                mt_v4i a;
                if (p < 6) {
                    a[0] = (int)((tc.x << (6 - p)) & 0x40404040u); a[1] = (int)((tc.y << (6 - p)) & 0x40404040u);
                    a[2] = (int)((tc.z << (6 - p)) & 0x40404040u); a[3] = (int)((tc.w << (6 - p)) & 0x40404040u);
                } else if (p == 6) {
                    a[0] = (int)(tc.x & 0x40404040u); a[1] = (int)(tc.y & 0x40404040u);
                    a[2] = (int)(tc.z & 0x40404040u); a[3] = (int)(tc.w & 0x40404040u);
                } else {
                    a[0] = (int)((tc.x >> 1) & 0x40404040u); a[1] = (int)((tc.y >> 1) & 0x40404040u);
                    a[2] = (int)((tc.z >> 1) & 0x40404040u); a[3] = (int)((tc.w >> 1) & 0x40404040u);
                }
#pragma unroll
                for (int c = 0; c < QT; ++c) acc[c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[c][p], acc[c], 0, 0, 0);
            }
            // best <= second always: the new second-smallest is the median of (best, second, key)  (one v_med3_i32)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
#pragma unroll
                for (int c = 0; c < QT; ++c) {
                    const int kc = acc[c][i];
                    second[c] = max(min(best[c], second[c]), min(max(best[c], second[c]), kc));
                    best[c] = min(best[c], kc);
                }
            }
        }
        // fold the chunk into the running result
#pragma unroll
        for (int c = 0; c < QT; ++c) {
            const uint32_t b = best[c] == 0x7fffffff ? 0xffffffffu
                                                     : ((uint32_t)((best[c] >> 12) + pq[c] - 256) << 20) | (uint32_t)(c0 + (best[c] & 4095));
            const uint32_t s2 = second[c] == 0x7fffffff ? 0xffffffffu
                                                        : ((uint32_t)((second[c] >> 12) + pq[c] - 256) << 20) | (uint32_t)(c0 + (second[c] & 4095));
            gsecond[c] = mt_min2(mt_min2(gsecond[c], s2), mt_max2(gbest[c], b));
            gbest[c] = mt_min2(gbest[c], b);
        }
    }
    if (!wave_on) return;
    // the two lane halves hold different train rows of the same query
#pragma unroll
    for (int c = 0; c < QT; ++c) {
        const uint32_t ob = (uint32_t)__shfl_xor((int)gbest[c], 32), os = (uint32_t)__shfl_xor((int)gsecond[c], 32);
        const uint32_t second = mt_min2(mt_min2(gsecond[c], os), mt_max2(gbest[c], ob));
        const uint32_t best = mt_min2(gbest[c], ob);
        const int qi = qw + 32 * c + r;
        if (h == 0 && qi < NQ) {
            if (nsplit > 1) {
                partial[((long long)pr * nsplit + sp) * out_stride + qi] = make_uint2(best, second);
            } else {
                const long long o = (long long)pr * out_stride + qi;
                best_idx[o] = best == 0xffffffffu ? -1 : (int)(best & 0xfffffu);
                best_dist[o] = best == 0xffffffffu ? 0x7fffffff : (int)(best >> 20);
                second_dist[o] = second == 0xffffffffu ? 0x7fffffff : (int)(second >> 20);
            }
        }
    }
}

// k_match on the FP4 rate of the matrix pipe (round 3).  The same bookkeeping, the same keys, the same result bits -- the
// products come from v_mfma_scale_f32_32x32x64_f8f6f4 with both operands in e2m1: a descriptor bit is the nibble 0b0100 (2.0)
// on the train side and 0b1110 (-4.0) on the query side, the block scale of the train operand is 2^10, so a common bit adds
// -8 * 2^10 = -2 << 12 to the accumulator, which is LOADED with the float of key(t) = (popc(t) + 256) << 12 | index.  Every
// partial sum is an integer below 2^24: exact in f32 (tools/mfma_fp4_probe.hip checks the instruction with such data, layout and
// scale bytes included).  K = 64 descriptor bits per instruction at the cycles of the 32-bit-K int8 form: four MFMAs per
// 32 x 32 distances instead of eight, and the expansion of a train tile is 28 instead of 60 vector instructions (bit 4j+k of a
// dword -> nibble j of register k: shift + and).  Positive floats order like their bit patterns, so best / second stay
// v_min_i32 / v_med3_i32 on the raw bits.
typedef int mt_v8i __attribute__((ext_vector_type(8)));
typedef float mt_v16f __attribute__((ext_vector_type(16)));
#define MT_F4_NONE 0x7f7fffff   // FLT_MAX: "no key yet" / rows past the end (a zero descriptor adds nothing to it)
#ifndef MT_F4_LB2
#define MT_F4_LB2 3
#endif
#ifndef MT_F4_LB4
#define MT_F4_LB4 2
#endif
template <int QT>
__global__ __launch_bounds__(64 * MT_WAVES, QT == 2 ? MT_F4_LB2 : MT_F4_LB4) void k_match_f4(const uint8_t *__restrict__ q, const int *__restrict__ nq,
                                                         long long q_stride, const uint8_t *__restrict__ t,
                                                         const int *__restrict__ nt, long long t_stride,
                                                         uint2 *__restrict__ partial, int *__restrict__ best_idx,
                                                         int *__restrict__ best_dist, int *__restrict__ second_dist,
                                                         int out_stride, int nsplit) {
    __shared__ __attribute__((aligned(16))) float s_tk[MT_CHUNK];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), pr = blockIdx.z, sp = blockIdx.y;
    const int NQ = min(nq[pr], out_stride), NT = min(nt[pr], 1 << 20);
    if ((int)blockIdx.x * MT_QPB(QT) >= NQ) return;
    const int r = lane & 31, h = lane >> 5;
    const uint8_t *qp = q + (long long)pr * q_stride;
    const uint8_t *tp = t + (long long)pr * t_stride;
    const int per = ((NT + 31) / 32 + nsplit - 1) / nsplit * 32;
    const int j0 = min(NT, sp * per), j1 = min(NT, j0 + per);
    // ---- queries: lane (r, h) holds bytes 16h .. 16h+15 of query r of each tile; dword p of them is the K block of MFMA p
    const int qw = blockIdx.x * MT_QPB(QT) + w * MT_QPW(QT);
    const bool wave_on = qw < NQ;
    mt_v4i bq[QT][4];
    int pq[QT];
#pragma unroll
    for (int c = 0; c < QT; ++c) {
        const int qi = qw + 32 * c + r;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (qi < NQ) v = *(const uint4 *)(qp + (long long)qi * 32 + 16 * h);
        pq[c] = __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
        pq[c] += __shfl_xor(pq[c], 32);
        const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t e = (vv[p] >> k) & 0x11111111u;
                bq[c][p][k] = (int)((e << 1) | (e << 2) | (e << 3));   // 0b1110 per set bit
            }
        }
    }
    uint32_t gbest[QT], gsecond[QT];
#pragma unroll
    for (int c = 0; c < QT; ++c) gbest[c] = gsecond[c] = 0xffffffffu;
    for (int c0 = j0; c0 < j1; c0 += MT_CHUNK) {
        const int c1 = min(j1, c0 + MT_CHUNK), n = c1 - c0, npad = (n + 31) & ~31;
        __syncthreads();
        for (int i = threadIdx.x; i < npad; i += 64 * MT_WAVES) {
            float key = __int_as_float(MT_F4_NONE);
            if (i < n) {
                const uint4 a = *(const uint4 *)(tp + (long long)(c0 + i) * 32), b = *(const uint4 *)(tp + (long long)(c0 + i) * 32 + 16);
                const int pt = __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(b.x) + __popc(b.y) + __popc(b.z) + __popc(b.w);
                key = (float)(((pt + 256) << 12) | i);   // < 2^24: exact
            }
            s_tk[i] = key;
        }
        __syncthreads();
        if (!wave_on) continue;
        int best[QT], second[QT];
#pragma unroll
        for (int c = 0; c < QT; ++c) best[c] = second[c] = MT_F4_NONE;
        const uint8_t *trow = tp + (long long)(c0 + r) * 32 + 16 * h;
        uint4 ta = make_uint4(0, 0, 0, 0);
        if (r < n) ta = *(const uint4 *)trow;
        for (int jt = 0; jt < npad; jt += 32) {
            const uint4 tc = ta;
            ta = make_uint4(0, 0, 0, 0);
            if (jt + 32 + r < n) ta = *(const uint4 *)(trow + (long long)(jt + 32) * 32);
            mt_v16f acc[QT];
            {
                const float4 *kp = (const float4 *)(s_tk + jt + 4 * h);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 k4 = kp[2 * g];
                    acc[0][4 * g] = k4.x; acc[0][4 * g + 1] = k4.y; acc[0][4 * g + 2] = k4.z; acc[0][4 * g + 3] = k4.w;
                }
#pragma unroll
                for (int c = 1; c < QT; ++c) acc[c] = acc[0];
            }
            const uint32_t tw[4] = {tc.x, tc.y, tc.z, tc.w};
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                mt_v8i a = {0, 0, 0, 0, 0, 0, 0, 0};
                a[0] = (int)((tw[p] << 2) & 0x44444444u); a[1] = (int)((tw[p] << 1) & 0x44444444u);
                a[2] = (int)(tw[p] & 0x44444444u);        a[3] = (int)((tw[p] >> 1) & 0x44444444u);
#pragma unroll
                for (int c = 0; c < QT; ++c) {
                    mt_v8i b = {0, 0, 0, 0, 0, 0, 0, 0};
                    b[0] = bq[c][p][0]; b[1] = bq[c][p][1]; b[2] = bq[c][p][2]; b[3] = bq[c][p][3];
                    acc[c] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc[c], 4, 4, 0, 137, 0, 127);
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
#pragma unroll
                for (int c = 0; c < QT; ++c) {
                    const int kc = __float_as_int(acc[c][i]);
                    second[c] = max(min(best[c], second[c]), min(max(best[c], second[c]), kc));
                    best[c] = min(best[c], kc);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < QT; ++c) {
            const int bk = (int)__int_as_float(best[c]), sk = (int)__int_as_float(second[c]);   // the integer keys (exact; unused when NONE)
            const uint32_t b = best[c] == MT_F4_NONE ? 0xffffffffu
                                                     : ((uint32_t)((bk >> 12) + pq[c] - 256) << 20) | (uint32_t)(c0 + (bk & 4095));
            const uint32_t s2 = second[c] == MT_F4_NONE ? 0xffffffffu
                                                        : ((uint32_t)((sk >> 12) + pq[c] - 256) << 20) | (uint32_t)(c0 + (sk & 4095));
            gsecond[c] = mt_min2(mt_min2(gsecond[c], s2), mt_max2(gbest[c], b));
            gbest[c] = mt_min2(gbest[c], b);
        }
    }
    if (!wave_on) return;
#pragma unroll
    for (int c = 0; c < QT; ++c) {
        const uint32_t ob = (uint32_t)__shfl_xor((int)gbest[c], 32), os = (uint32_t)__shfl_xor((int)gsecond[c], 32);
        const uint32_t second = mt_min2(mt_min2(gsecond[c], os), mt_max2(gbest[c], ob));
        const uint32_t best = mt_min2(gbest[c], ob);
        const int qi = qw + 32 * c + r;
        if (h == 0 && qi < NQ) {
            if (nsplit > 1) {
                partial[((long long)pr * nsplit + sp) * out_stride + qi] = make_uint2(best, second);
            } else {
                const long long o = (long long)pr * out_stride + qi;
                best_idx[o] = best == 0xffffffffu ? -1 : (int)(best & 0xfffffu);
                best_dist[o] = best == 0xffffffffu ? 0x7fffffff : (int)(best >> 20);
                second_dist[o] = second == 0xffffffffu ? 0x7fffffff : (int)(second >> 20);
            }
        }
    }
}

// The same bookkeeping on the vector pipe (the round-1 kernel, ORBX_MATCH_KERNEL=valu): two queries per lane (16 dwords in
// VGPRs); the train descriptor of an iteration is the same for the whole wave, so it is fetched with SCALAR loads
// (s_load_dwordx8 through the scalar cache) and used as the SGPR operand of v_xor: no LDS staging, no barrier.  19 vector
// instructions per pair of distances; partial results always go through k_match_merge.
__global__ __launch_bounds__(64) void k_match_valu(const uint8_t *__restrict__ q, const int *__restrict__ nq,
                                                         long long q_stride, const uint8_t *__restrict__ t,
                                                         const int *__restrict__ nt, long long t_stride,
                                                         uint2 *__restrict__ partial, int out_stride, int nsplit) {
    // key = dist << 20 | index: min(key) is the best match with the lowest index on ties; the second-smallest
    // key carries the second-best distance (counting duplicates), exactly the bookkeeping of the reference loops.
    const int lane = threadIdx.x, pr = blockIdx.z, sp = blockIdx.y;
    const int NQ = min(nq[pr], out_stride), NT = min(nt[pr], 1 << 20);   // contract (orbx.h): counts beyond out_stride are ignored
    const int qw = blockIdx.x * 128;
    if (qw >= NQ) return;
    const int qi0 = qw + lane, qi1 = qi0 + 64;
    const uint4 *qp = (const uint4 *)(q + (long long)pr * q_stride);
    const uint4 *tp = (const uint4 *)(t + (long long)pr * t_stride);
    uint4 qa0 = make_uint4(0, 0, 0, 0), qb0 = qa0, qa1 = qa0, qb1 = qa0;
    if (qi0 < NQ) { qa0 = qp[2 * qi0]; qb0 = qp[2 * qi0 + 1]; }
    if (qi1 < NQ) { qa1 = qp[2 * qi1]; qb1 = qp[2 * qi1 + 1]; }
    const int chunk = (NT + nsplit - 1) / nsplit;
    const int j0 = sp * chunk, j1 = min(NT, j0 + chunk);
    uint32_t best0 = 0xffffffffu, second0 = 0xffffffffu, best1 = 0xffffffffu, second1 = 0xffffffffu;
#pragma unroll 4
    for (int j = j0; j < j1; ++j) {
        const uint4 ta = tp[2 * j], tb = tp[2 * j + 1];   // wave-uniform address: scalar loads
        const uint32_t d0 = __popc(qa0.x ^ ta.x) + __popc(qa0.y ^ ta.y) + __popc(qa0.z ^ ta.z) + __popc(qa0.w ^ ta.w) +
                            __popc(qb0.x ^ tb.x) + __popc(qb0.y ^ tb.y) + __popc(qb0.z ^ tb.z) + __popc(qb0.w ^ tb.w);
        const uint32_t d1 = __popc(qa1.x ^ ta.x) + __popc(qa1.y ^ ta.y) + __popc(qa1.z ^ ta.z) + __popc(qa1.w ^ ta.w) +
                            __popc(qb1.x ^ tb.x) + __popc(qb1.y ^ tb.y) + __popc(qb1.z ^ tb.z) + __popc(qb1.w ^ tb.w);
        const uint32_t key0 = (d0 << 20) | (uint32_t)j, key1 = (d1 << 20) | (uint32_t)j;
        // best <= second always: the new second-smallest is the median of (best, second, key)  (one v_med3_u32)
        second0 = max(min(best0, second0), min(max(best0, second0), key0));
        best0 = min(best0, key0);
        second1 = max(min(best1, second1), min(max(best1, second1), key1));
        best1 = min(best1, key1);
    }
    uint2 *po = partial + ((long long)pr * nsplit + sp) * out_stride;
    if (qi0 < NQ) po[qi0] = make_uint2(best0, second0);
    if (qi1 < NQ) po[qi1] = make_uint2(best1, second1);
}

__global__ __launch_bounds__(256) void k_match_merge(const int *__restrict__ nq, const uint2 *__restrict__ partial,
                                                     int *__restrict__ best_idx, int *__restrict__ best_dist,
                                                     int *__restrict__ second_dist, int out_stride, int nsplit) {
    const int pr = blockIdx.y, qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= min(nq[pr], out_stride)) return;
    uint32_t best = 0xffffffffu, second = 0xffffffffu;
    for (int k = 0; k < nsplit; ++k) {
        const uint2 p = partial[((long long)pr * nsplit + k) * out_stride + qi];
        second = min(min(second, p.y), max(best, p.x));
        best = min(best, p.x);
    }
    const long long o = (long long)pr * out_stride + qi;
    best_idx[o] = best == 0xffffffffu ? -1 : (int)(best & 0xfffffu);
    best_dist[o] = best == 0xffffffffu ? 0x7fffffff : (int)(best >> 20);
    second_dist[o] = second == 0xffffffffu ? 0x7fffffff : (int)(second >> 20);
}

// full distance matrix (uint16) for host-side sequential policies
__global__ __launch_bounds__(256) void k_hamming_matrix(const uint8_t *__restrict__ q, int nq,
                                                        const uint8_t *__restrict__ t, int nt,
                                                        uint16_t *__restrict__ dist) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nq * nt) return;
    const int qi = (int)(i / nt), ti = (int)(i - (long long)qi * nt);
    const uint4 *qp = (const uint4 *)q + 2 * qi, *tp = (const uint4 *)t + 2 * ti;
    const uint4 qa = qp[0], qb = qp[1], ta = tp[0], tb = tp[1];
    dist[i] = (uint16_t)(__popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                         __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w));
}

// ------------------------------------------------------------------------------------------------
// K8: Frame::ComputeStereoMatches (reference src/Frame.cc:880-1176), one wave per LEFT keypoint.
//  phase A: every lane scans right keypoints (stride 64); the reference's row table (:926-942) is the predicate
//           floor(yR - r) <= (int)vL <= ceil(yR + r) with r = 2*scale[octaveR]; candidates are visited in ascending
//           index, so min over key = dist << 16 | iR reproduces the strict '<' bookkeeping (:990-1018).
//  phase B: 11x11 patch vs 11 shifts, centre-subtracted L1 (:1040-1101) in exact integer arithmetic; the
//           parabola (:1121-1129) uses the same single-rounded float operations as the reference.
// The final median cut (:1160-1175) is a sort over <= N integers and stays on the host (orbx_pyramid.cpp).
// ------------------------------------------------------------------------------------------------
// 16 lanes per LEFT keypoint, four keypoints per wave: every cross-lane step (candidate minimum, the 11 SAD sums) is a DPP
// rotate inside a row of 16 lanes and serves four keypoints at once, and a wave's chain of dependent loads (keypoint -> row
// table -> candidates -> descriptors -> best match -> patches) is paid once per four keypoints.  (One wave per keypoint: 330 us
// per 256 KITTI pairs, 11 x 7 DPP steps and a 5 us load chain per keypoint.)
__device__ __forceinline__ uint32_t st_row16_min(uint32_t v) {   // all-reduce min inside each row of 16 lanes
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x121, 0xf, 0xf, false));   // row_ror:1
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x122, 0xf, 0xf, false));   // row_ror:2
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x124, 0xf, 0xf, false));   // row_ror:4
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128, 0xf, 0xf, false));   // row_ror:8
    return v;
}
__device__ __forceinline__ uint32_t st_row16_sum(uint32_t v) {   // all-reduce sum inside each row of 16 lanes
    v += (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x121, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x122, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x124, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128, 0xf, 0xf, false);
    return v;
}
#define ST_KPB 16   // left keypoints per 256-thread block
__device__ __forceinline__ void orbx_stereo_body(const OrbxStereoGeom &sg, const orbx_keypoint *__restrict__ kL,
                                                 const uint8_t *__restrict__ dL, int nL,
                                                 const orbx_keypoint *__restrict__ kR,
                                                 const uint8_t *__restrict__ dR, int nR,
                                                 const uint8_t *__restrict__ pyrL, const uint8_t *__restrict__ pyrR,
                                                 float *__restrict__ uRight, float *__restrict__ depth,
                                                 int *__restrict__ sad, const int *__restrict__ row_begin,
                                                 const uint2 *__restrict__ row_items) {
    // No lane leaves early: the reductions below are DPP operations every lane of the wave takes part in; a keypoint that
    // drops out (`act`) just stops contributing.
    const int l16 = threadIdx.x & 15;
    const int iL = blockIdx.x * ST_KPB + (threadIdx.x >> 4);
    bool act = iL < nL;
    float uL = 0.f, vL = 0.f;
    int levelL = 0;
    if (act) { const orbx_keypoint kp = kL[iL]; uL = kp.x; vL = kp.y; levelL = kp.octave; }
    if (act && l16 == 0) { uRight[iL] = -1.0f; depth[iL] = -1.0f; sad[iL] = -1; }
    const long long row = (long long)vL;
    act = act && row >= 0 && row < sg.nrows0;                 // F6 clamp (reference: out-of-bounds index)
    const float maxD = sg.mbf / sg.mb, minD = 0.f;
    const float minU = uL - maxD, maxU = uL - minD;
    act = act && !(maxU < 0);
    uint4 qa = make_uint4(0, 0, 0, 0), qb = qa;
    if (act) { const uint4 *qp = (const uint4 *)(dL + (long long)iL * 32); qa = qp[0]; qb = qp[1]; }
    uint32_t best = 0xffffffffu;
    if (row_begin) {
        // vRowIndices[vL] of the reference (:926-942), built on the device by k_stereo_rows: only the right keypoints whose
        // row band covers this row are visited (their order does not matter: ties go to the smallest index, as the
        // reference's strict '<' over ascending iR resolves them)
        int j = 0, j1 = 0;
        if (act) { j = row_begin[row] + l16; j1 = row_begin[row + 1]; }
        for (; j < j1; j += 16) {
            // a table entry carries what the gate needs (x, index | octave << 16): one coalesced 8-byte load per lane
            // instead of a scattered read of the 28-byte keypoint record
            const uint2 it = row_items[j];
            const int iR = (int)(it.y & 0xffffu), octR = (int)(it.y >> 16);
            const float xR = __uint_as_float(it.x);
            const bool cand = (int)(octR >= levelL - 1) & (int)(octR <= levelL + 1) & (int)(xR >= minU) & (int)(xR <= maxU);
            if (cand) {
                const uint4 *tp = (const uint4 *)(dR + (long long)iR * 32);
                const uint4 ta = tp[0], tb = tp[1];
                const uint32_t d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                                   __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
                if (d < 100u) best = min(best, (d << 16) | (uint32_t)iR);
            }
        }
    } else {
        for (int iR = act ? l16 : nR; iR < nR; iR += 16) {
            const orbx_keypoint kr = kR[iR];
            const float r = 2.0f * sg.scale[kr.octave];
            const int maxr = (int)ceilf(kr.y + r), minr = (int)floorf(kr.y - r);
            const bool cand = (int)(row >= minr) & (int)(row <= maxr) & (int)(kr.octave >= levelL - 1) &
                              (int)(kr.octave <= levelL + 1) & (int)(kr.x >= minU) & (int)(kr.x <= maxU);
            if (cand) {
                const uint4 *tp = (const uint4 *)(dR + (long long)iR * 32);
                const uint4 ta = tp[0], tb = tp[1];
                const uint32_t d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                                   __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
                if (d < 100u) best = min(best, (d << 16) | (uint32_t)iR);   // bestDist starts at TH_HIGH, strict '<'
            }
        }
    }
    best = st_row16_min(best);
    act = act && best != 0xffffffffu && (best >> 16) < 75u;   // thOrbDist = (TH_HIGH + TH_LOW) / 2
    const int bestIdxR = act ? (int)(best & 0xffffu) : 0;
    float uR0 = 0.f;
    if (act) uR0 = kR[bestIdxR].x;
    const float scaleFactor = sg.inv_scale[levelL];
    const float scaleduL = roundf(uL * scaleFactor), scaledvL = roundf(vL * scaleFactor);
    const float scaleduR0 = roundf(uR0 * scaleFactor);
    const int w = 5, Lh = 5;
    const int W = sg.pw[levelL], H = sg.ph[levelL], pitch = sg.pitch[levelL];
    const int y0 = (int)(scaledvL - w), x0 = (int)(scaleduL - w);
    act = act && !(y0 < 0 || y0 + 2 * w + 1 > H || x0 < 0 || x0 + 2 * w + 1 > W);
    const float iniu = scaleduR0 - Lh - w, endu = scaleduR0 + Lh + w + 1;   // fork: minus (src/Frame.cc:1067)
    act = act && !(iniu < 0 || endu >= W);
    // ---- 11 x 11 patch against 11 shifts: SAD_s = sum |(L - cL) - (R[+s] - cR_s)| = sum |(L + cR_s - cL + 511) - (R[+s] + 511)|
    // (both sides non-negative 16-bit values).  Two pixels per lane and round in the 16-bit halves of a register: v_perm
    // picks byte s of both pixels' 12-byte windows of the right image, v_sad_u16 accumulates.  The centre pixel contributes 0 to every shift by construction, so the 7
    // slots beyond the 121 pixels of the 128 a group walks are filled with it.
    uint32_t acc[11];
#pragma unroll
    for (int s = 0; s < 11; ++s) acc[s] = 0u;
    if (act) {
        const uint8_t *IL = pyrL + sg.off[levelL] + (long long)y0 * pitch + x0;
        const uint8_t *IR = pyrR + sg.off[levelL] + (long long)y0 * pitch + ((int)scaleduR0 - w);
        const uint32_t cL = IL[w * pitch + w];
        const orbx_uint3_u cw = *(const orbx_uint3_u *)(IR + w * pitch);   // cR_s = IR[w * pitch + w + (s - Lh)] = byte s
        uint32_t Cs[11];
#pragma unroll
        for (int s = 0; s < 11; ++s) {
            const uint32_t cwd = s < 4 ? cw.x : s < 8 ? cw.y : cw.z;
            Cs[s] = (((cwd >> (8 * (s & 3))) & 0xffu) + 511u - cL) * 0x10001u;   // cR_s - cL + 511 in both halves (256 .. 766)
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int q0 = l16 + 16 * k, q1 = q0 + 64;
            if (q1 >= 121) q1 = 60;                           // the centre pixel: |0 - 0| for every shift
            const int y_0 = q0 / 11, x_0 = q0 - 11 * y_0, y_1 = q1 / 11, x_1 = q1 - 11 * y_1;
            const uint32_t L0 = IL[y_0 * pitch + x_0], L1 = IL[y_1 * pitch + x_1];
            const orbx_uint3_u r0 = *(const orbx_uint3_u *)(IR + y_0 * pitch + x_0 - Lh);   // R bytes x - 5 .. x + 6 of the row
            const orbx_uint3_u r1 = *(const orbx_uint3_u *)(IR + y_1 * pitch + x_1 - Lh);
            const uint32_t A0 = L0 | (L1 << 16);               // + Cs[s] = L + cR_s - cL + 511 in both halves (256 .. 1021)
#pragma unroll
            for (int s = 0; s < 11; ++s) {
                const uint32_t lo = s < 4 ? r0.x : s < 8 ? r0.y : r0.z, hi = s < 4 ? r1.x : s < 8 ? r1.y : r1.z;
                const uint32_t sel = (uint32_t)(s & 3) | (0x0cu << 8) | ((uint32_t)(4 + (s & 3)) << 16) | (0x0cu << 24);
                const uint32_t B = __builtin_amdgcn_perm(hi, lo, sel) + 0x01ff01ffu;   // R + 511 in both halves
                acc[s] = __builtin_amdgcn_sad_u16(A0 + Cs[s], B, acc[s]);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 11; ++s) acc[s] = st_row16_sum(acc[s]);
    if (!act || l16 != 0) return;
    int bestDistS = 0x7fffffff, bestinc = 0;
#pragma unroll
    for (int s = 0; s < 11; ++s)
        if ((int)acc[s] < bestDistS) { bestDistS = (int)acc[s]; bestinc = s - Lh; }
    if (bestinc == -Lh || bestinc == Lh) return;
    float dist1 = 0.f, dist2 = 0.f, dist3 = 0.f;
#pragma unroll
    for (int s = 1; s < 10; ++s)
        if (s - Lh == bestinc) { dist1 = (float)(int)acc[s - 1]; dist2 = (float)(int)acc[s]; dist3 = (float)(int)acc[s + 1]; }
    const float deltaR = (dist1 - dist3) / (2.0f * (dist1 + dist3 - 2.0f * dist2));
    if (deltaR < -1 || deltaR > 1) return;
    float bestuR = sg.scale[levelL] * ((float)scaleduR0 + (float)bestinc + deltaR);
    float disparity = uL - bestuR;
    if (disparity >= minD && disparity < maxD) {
        if (disparity <= 0) { disparity = (float)0.01; bestuR = (float)((double)uL - 0.01); }
        depth[iL] = sg.mbf / disparity;
        uRight[iL] = bestuR;
        sad[iL] = bestDistS;
    }
}

__global__ __launch_bounds__(256) void k_stereo(OrbxStereoGeom sg, const orbx_keypoint *__restrict__ kL,
                                                const uint8_t *__restrict__ dL, int nL,
                                                const orbx_keypoint *__restrict__ kR,
                                                const uint8_t *__restrict__ dR, int nR,
                                                const uint8_t *__restrict__ pyrL, const uint8_t *__restrict__ pyrR,
                                                float *__restrict__ uRight, float *__restrict__ depth,
                                                int *__restrict__ sad, const int *__restrict__ row_begin,
                                                const uint2 *__restrict__ row_items) {
    orbx_stereo_body(sg, kL, dL, nL, kR, dR, nR, pyrL, pyrR, uRight, depth, sad, row_begin, row_items);
}
// batched: blockIdx.y = stereo pair; keypoints / descriptors / results of pair p at p * cap, pyramids at p * pyr_bytes
__global__ __launch_bounds__(256) void k_stereo_batch(OrbxStereoGeom sg, const orbx_keypoint *__restrict__ kL,
                                                      const uint8_t *__restrict__ dL, const int *__restrict__ nL,
                                                      const orbx_keypoint *__restrict__ kR,
                                                      const uint8_t *__restrict__ dR, const int *__restrict__ nR, int cap,
                                                      const uint8_t *__restrict__ pyrL, const uint8_t *__restrict__ pyrR,
                                                      long long pyr_bytes, float *__restrict__ uRight,
                                                      float *__restrict__ depth, int *__restrict__ sad,
                                                      const int *__restrict__ row_begin, const uint2 *__restrict__ row_items,
                                                      int items_per_pair) {
    const long long p = blockIdx.y;
    orbx_stereo_body(sg, kL + p * cap, dL + p * cap * 32, min(nL[p], cap), kR + p * cap, dR + p * cap * 32, min(nR[p], cap),
                     pyrL + p * pyr_bytes, pyrR + p * pyr_bytes, uRight + p * cap, depth + p * cap, sad + p * cap,
                     row_begin ? row_begin + p * (sg.nrows0 + 1) : nullptr, row_items ? row_items + p * items_per_pair : nullptr);
}
// vRowIndices of Frame::ComputeStereoMatches (src/Frame.cc:926-942) for one stereo pair per workgroup: right keypoint iR is
// listed under every row of [floor(y - r), ceil(y + r)], r = 2 * mvScaleFactors[octave] (rows outside the image are clamped
// away: the reference indexes out of bounds there).  Histogram, scan and fill all in LDS; rows <= ST_MAX_ROWS.
#define ST_MAX_ROWS 4096
__global__ __launch_bounds__(1024) void k_stereo_rows(OrbxStereoGeom sg, const orbx_keypoint *__restrict__ kR,
                                                      const int *__restrict__ nR, int cap, int *__restrict__ row_begin,
                                                      uint2 *__restrict__ row_items, int items_per_pair, int n_direct) {
    __shared__ int s_cnt[ST_MAX_ROWS + 1];
    __shared__ int s_part[1024];
    const long long p = blockIdx.x;
    const int t = threadIdx.x, n = nR ? min(nR[p], cap) : n_direct, rows = sg.nrows0;   // (single pair: the count comes by value)
    const orbx_keypoint *k = kR + p * cap;
    for (int i = t; i <= rows; i += 1024) s_cnt[i] = 0;
    __syncthreads();
    for (int i = t; i < n; i += 1024) {
        const float r = 2.0f * sg.scale[k[i].octave];
        const int maxr = min((int)ceilf(k[i].y + r), rows - 1), minr = max((int)floorf(k[i].y - r), 0);
        for (int y = minr; y <= maxr; ++y) atomicAdd(&s_cnt[y], 1);
    }
    __syncthreads();
    // exclusive scan over the rows: each thread owns a contiguous chunk
    const int chunk = (rows + 1023) / 1024, r0 = t * chunk, r1 = min(r0 + chunk, rows);
    int sum = 0;
    for (int y = r0; y < r1; ++y) sum += s_cnt[y];
    s_part[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = t >= o ? s_part[t - o] : 0;
        __syncthreads();
        s_part[t] += v;
        __syncthreads();
    }
    int run = s_part[t] - sum;
    int *rb = row_begin + p * (rows + 1);
    for (int y = r0; y < r1; ++y) { const int c = s_cnt[y]; s_cnt[y] = run; rb[y] = run; run += c; }
    if (t == 1023) rb[rows] = s_part[1023];
    __syncthreads();
    uint2 *items = row_items + p * items_per_pair;
    for (int i = t; i < n; i += 1024) {
        const float r = 2.0f * sg.scale[k[i].octave];
        const int maxr = min((int)ceilf(k[i].y + r), rows - 1), minr = max((int)floorf(k[i].y - r), 0);
        for (int y = minr; y <= maxr; ++y) {
            const int pos = atomicAdd(&s_cnt[y], 1);
            if (pos < items_per_pair) items[pos] = make_uint2(__float_as_uint(k[i].x), (uint32_t)i | ((uint32_t)k[i].octave << 16));
        }
    }
}
// Median cut of Frame::ComputeStereoMatches (src/Frame.cc:1160-1175) on the device, one workgroup per pair: the reference
// sorts (SAD, index) and drops everything with SAD >= 1.5f * 1.4f * median, median = element size/2 of the sorted list.
// Only the VALUE of that element matters: two 256-bin histogram passes over the 16-bit SAD (<= 121 * 510) select it.
// (the two selections over the 256 bins are block-wide prefix sums -- one wave scan + four wave totals -- not a serial walk by
// one thread: 21 -> 6 us per 64 KITTI pairs)
__global__ __launch_bounds__(256) void k_stereo_cut(const int *__restrict__ nL, int cap, const int *__restrict__ sad,
                                                    float *__restrict__ uRight, float *__restrict__ depth,
                                                    int *__restrict__ nmatches) {
    __shared__ int hist[256];
    __shared__ int wsum[4];
    __shared__ int s_sel, s_rank, s_kept;
    const long long p = blockIdx.x;
    const int n = min(nL[p], cap), t = threadIdx.x, wv = t >> 6;
    const int *sd = sad + p * cap;
    float *ur = uRight + p * cap, *dp = depth + p * cap;
    hist[t] = 0;
    if (t == 0) { s_kept = 0; s_sel = -1; s_rank = 0; }
    __syncthreads();
    for (int i = t; i < n; i += 256) { const int v = sd[i]; if (v >= 0) atomicAdd(&hist[(v >> 8) & 255], 1); }
    __syncthreads();
    // bin that holds the element of rank k = count / 2 (nth_element semantics of :1160-1165), and the rank inside it
    int v = hist[t];
    int incl = orbx_wave_scan(v);
    if ((t & 63) == 63) wsum[wv] = incl;
    __syncthreads();
    const int cnt = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    for (int i = 0; i < wv; ++i) incl += wsum[i];
    if (cnt > 0) {
        const int k = cnt / 2;
        if (incl - v <= k && k < incl) { s_sel = t; s_rank = k - (incl - v); }
    }
    if (t == 0) s_kept = cnt;
    __syncthreads();
    const int hi = s_sel, rank = s_rank;
    if (hi < 0) { if (t == 0) nmatches[p] = 0; return; }
    __syncthreads();
    hist[t] = 0;
    __syncthreads();
    for (int i = t; i < n; i += 256) { const int u = sd[i]; if (u >= 0 && ((u >> 8) & 255) == hi) atomicAdd(&hist[u & 255], 1); }
    __syncthreads();
    v = hist[t];
    incl = orbx_wave_scan(v);
    if ((t & 63) == 63) wsum[wv] = incl;
    __syncthreads();
    for (int i = 0; i < wv; ++i) incl += wsum[i];
    if (incl - v <= rank && rank < incl) s_sel = (hi << 8) | t;
    __syncthreads();
    const float median = (float)s_sel;
    const float thDist = 1.5f * 1.4f * median;
    int dropped = 0;
    for (int i = t; i < n; i += 256) {
        const int u = sd[i];
        if (u >= 0 && (float)u >= thDist) { ur[i] = -1.0f; dp[i] = -1.0f; ++dropped; }
    }
    if (dropped) atomicSub(&s_kept, dropped);
    __syncthreads();
    if (t == 0) nmatches[p] = s_kept;
}

// small helper: zero per-batch counters / status
// ------------------------------------------------------------------------------------------------
// K9: DBoW2 TemplatedVocabulary<FORB>::transform(feature, word_id, weight, nid, levelsup)
// (reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1240-1285, FORB::distance FORB.cpp:81-101; caller
// Frame::ComputeBoW src/Frame.cc:750-765 with levelsup = 4).  16 lanes per descriptor: lane c takes child c of the current
// node (k <= 20 in every loadable vocabulary: one or two rounds), XOR + popcount over the 8 dwords, then a rotate-reduce
// inside the 16-lane DPP row on the key (distance << 16 | position) -- the minimum is the FIRST closest child, as the
// reference's strict '<' scan picks it.  Outputs the leaf node and the node at depth L - levelsup; word id and weight are
// table look-ups the host does in double precision.
// ------------------------------------------------------------------------------------------------
struct DVoc {
    const int *child_begin;       // n_nodes + 1 offsets into child_ids (Node::children in vector order)
    const uint32_t *child_ids;
    const uint8_t *desc;          // n_nodes x 32
    int n_nodes, L;
};
__device__ __forceinline__ uint32_t orbx_row16_min(uint32_t v) {   // all-reduce min inside each row of 16 lanes
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x121, 0xf, 0xf, false));   // row_ror:1
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x122, 0xf, 0xf, false));   // row_ror:2
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x124, 0xf, 0xf, false));   // row_ror:4
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128, 0xf, 0xf, false));   // row_ror:8
    return v;
}
__global__ __launch_bounds__(256) void k_bow_transform(DVoc voc, const uint8_t *__restrict__ desc,
                                                       const int *__restrict__ counts, long long frame_stride, int levelsup,
                                                       uint32_t *__restrict__ out_leaf, uint32_t *__restrict__ out_nid,
                                                       int out_stride) {
    const int sub = threadIdx.x & 15;
    const int feat = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int f = blockIdx.y;
    const int n = counts[f];
    // inactive groups keep walking a dummy descriptor: the DPP reduction wants whole rows executing together
    const bool live = feat < n;
    const uint4 *q = (const uint4 *)(desc + (long long)f * frame_stride + (long long)(live ? feat : 0) * 32);
    const uint4 qa = n > 0 ? q[0] : make_uint4(0, 0, 0, 0), qb = n > 0 ? q[1] : make_uint4(0, 0, 0, 0);
    const int nid_level = voc.L - levelsup;
    uint32_t node = 0, nid = 0;
    for (int level = 1; level <= 64; ++level) {   // child ids exceed their parent's (checked on the host): terminates
        const int cb = voc.child_begin[node], ce = voc.child_begin[node + 1];
        if (cb == ce) break;                      // leaf
        uint32_t best = 0xffffffffu;
        for (int c0 = cb; c0 < ce; c0 += 16) {
            const int c = c0 + sub;
            uint32_t key = 0xffffffffu;
            if (c < ce) {
                const uint4 *t = (const uint4 *)(voc.desc + (long long)voc.child_ids[c] * 32);
                const uint4 ta = t[0], tb = t[1];
                const uint32_t d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                                   __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
                key = (d << 16) | (uint32_t)(c - cb);
            }
            best = min(best, orbx_row16_min(key));
        }
        node = voc.child_ids[cb + (int)(best & 0xffffu)];
        if (level == nid_level) nid = node;
    }
    if (live && sub == 0) {
        out_leaf[(long long)f * out_stride + feat] = node;
        out_nid[(long long)f * out_stride + feat] = nid;
    }
}

// ------------------------------------------------------------------------------------------------
// K10: Frame::UndistortKeyPoints (reference src/Frame.cc:770-825) = cv::undistortPoints(K, D, R = I, P = K) on the
// keypoint coordinates (OpenCV 3.2 cvUndistortPoints: double precision, five fixed iterations; parity unpinned, see
// oracle/orb_oracle_match.c).  One thread per keypoint, the other 20 bytes of the record are copied.
// ------------------------------------------------------------------------------------------------
struct DUndist { double fx, fy, cx, cy, k[14]; int identity; };
// the per-keypoint body of K10, shared with k_rgbd (K10b): both write the same undistorted record
__device__ __forceinline__ void undistort_kp(const DUndist &u, orbx_keypoint &kp) {
    if (!u.identity) {
        const double ifx = 1. / u.fx, ify = 1. / u.fy;
        double x = (double)kp.x, y = (double)kp.y;
        const double x0 = x = (x - u.cx) * ifx;
        const double y0 = y = (y - u.cy) * ify;
        for (int j = 0; j < 5; ++j) {
            const double r2 = x * x + y * y;
            const double icdist = (1 + ((u.k[7] * r2 + u.k[6]) * r2 + u.k[5]) * r2) / (1 + ((u.k[4] * r2 + u.k[1]) * r2 + u.k[0]) * r2);
            const double deltaX = 2 * u.k[2] * x * y + u.k[3] * (r2 + 2 * x * x) + u.k[8] * r2 + u.k[9] * r2 * r2;
            const double deltaY = u.k[2] * (r2 + 2 * y * y) + 2 * u.k[3] * x * y + u.k[10] * r2 + u.k[11] * r2 * r2;
            x = (x0 - deltaX) * icdist;
            y = (y0 - deltaY) * icdist;
        }
        const double xx = u.fx * x + 0.0 * y + u.cx, yy = 0.0 * x + u.fy * y + u.cy;
        const double ww = 1. / (0.0 * x + 0.0 * y + 1.0);
        kp.x = (float)(xx * ww);
        kp.y = (float)(yy * ww);
    }
}
__global__ __launch_bounds__(256) void k_undistort(DUndist u, const orbx_keypoint *__restrict__ kps, const int *__restrict__ counts,
                                                   int fixed_n, int cap, orbx_keypoint *__restrict__ out) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = counts ? min(counts[f], cap) : fixed_n;
    if (i >= n) return;
    orbx_keypoint kp = kps[(long long)f * cap + i];
    undistort_kp(u, kp);
    out[(long long)f * cap + i] = kp;
}

// ------------------------------------------------------------------------------------------------
// K10b: the RGB-D Frame (reference src/Frame.cc:237-321): Frame::ComputeStereoFromRGBD (:1179-1226) fused with K10.  One
// thread per keypoint: mvKeysUn (the record k_undistort writes, or read from `kun_in` when the caller has it already), then
// the depth sample at the DISTORTED keypoint, u = (int)kp.x, v = (int)kp.y, read where the reference reads it: byte
// o = v * pitch + 4 * u of the float image Tracking::GrabImageRGBD made (src/Tracking.cc:327-332; pitch = 4 * W for u16 input,
// which convertTo turned into a continuous float image, the caller's stride for f32 input).  A u beyond the row wraps into the
// next row, as in the reference (the coordinates are padded-image coordinates).  F7: a sample with o + 4 > limit =
// (H - 1) * pitch + 4 * W lies past the image's memory (undefined behaviour in the reference) and gives no depth; so do
// negative, non-finite and too-large coordinates, rejected before the integer conversion.  d > 0: mvDepth = d, mvuRight =
// xU - mbf / d (IEEE single division, no contraction: the build has -ffp-contract=off); otherwise both stay -1.
// ------------------------------------------------------------------------------------------------
struct DRgbd {
    const uint8_t *depth;       // frame 0 of the depth input
    long long frame_stride;     // bytes between frames
    long long stride;           // bytes per row of the input (u16 or f32)
    long long pitch;            // bytes per row of the float image the reference reads
    long long limit;            // (H - 1) * pitch + 4 * W
    int W, u16, scale_rows;     // scale_rows: f32 input converted in place (only the W floats of each row are scaled)
    float scale, mbf;
};
__global__ __launch_bounds__(256) void k_rgbd(DUndist u, DRgbd r, const orbx_keypoint *__restrict__ kps,
                                              const orbx_keypoint *__restrict__ kun_in, const int *__restrict__ counts, int fixed_n,
                                              int cap, orbx_keypoint *__restrict__ kun_out, float *__restrict__ u_right,
                                              float *__restrict__ depth) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = counts ? min(counts[f], cap) : fixed_n;
    if (i >= n) return;
    const long long at = (long long)f * cap + i;
    const orbx_keypoint kp = kps[at];
    float xu;
    if (kun_in) {
        xu = kun_in[at].x;
    } else {
        orbx_keypoint ku = kp;
        undistort_kp(u, ku);
        if (kun_out) kun_out[at] = ku;
        xu = ku.x;
    }
    float ur = -1.0f, dd = -1.0f;
    // NaN fails both comparisons; 2^31 keeps the conversion defined
    if (kp.x >= 0.0f && kp.y >= 0.0f && kp.x < 2147483648.0f && kp.y < 2147483648.0f) {
        const long long uu = (int)kp.x, vv = (int)kp.y;
        const long long o = vv * r.pitch + 4 * uu;
        if (o + 4 <= r.limit) {
            const uint8_t *img = r.depth + (long long)f * r.frame_stride;
            float d;
            if (r.u16) {   // cvtScale_ (OpenCV 3.2): one float multiply, then + 0.0f
                const long long p = o >> 2, row = p / r.W, col = p - row * r.W;
                d = (float)*(const uint16_t *)(img + row * r.stride + 2 * col) * r.scale + 0.0f;
            } else {
                d = *(const float *)(img + o);
                if (r.scale_rows && o % r.pitch < 4LL * r.W) d = d * r.scale + 0.0f;   // the gap between rows stays unscaled
            }
            if (d > 0.0f) {
                dd = d;
                ur = xu - r.mbf / d;
            }
        }
    }
    u_right[at] = ur;
    depth[at] = dd;
}

// ------------------------------------------------------------------------------------------------
// K11: the Frame grid on the device.  k_grid_build = Frame::AssignFeaturesToGrid + PosInGrid (reference src/Frame.cc:432-460,
// 729-745): 64 x 48 buckets, every bucket lists its features in ascending feature index (push_back order).  k_gate =
// Frame::GetFeaturesInArea (:633-717) for one query per wave, fused with DescriptorDistance: the cells are walked in the
// reference's order (ix outer, iy inner -- for one ix the buckets iy0..iy1 are one contiguous range of the CSR item
// array), the radius / level tests (incl. the quirk `bCheckLevels = minLevel > 0 || maxLevel >= 0`, :673) run per lane,
// survivors are ballot-compacted in visiting order and leave as (feature index | Hamming distance << 16).  The policies'
// order-dependent bookkeeping reads these short lists on the host instead of a dense nq x nt distance matrix.
// ------------------------------------------------------------------------------------------------
#define GR_COLS 64
#define GR_ROWS 48
#define GR_CELLS (GR_COLS * GR_ROWS)
__device__ __forceinline__ int gr_cell_of(const DGrid &gp, const orbx_keypoint &kp) {
    const int px = (int)roundf((kp.x - gp.minx) * gp.winv), py = (int)roundf((kp.y - gp.miny) * gp.hinv);   // C round(): half away from zero
    return (px < 0 || px >= GR_COLS || py < 0 || py >= GR_ROWS) ? -1 : px * GR_ROWS + py;
}
__global__ __launch_bounds__(1024) void k_grid_build(DGrid gp, const orbx_keypoint *__restrict__ kps, const int *__restrict__ counts,
                                                     int fixed_n, int cap, int *__restrict__ cell_begin, uint16_t *__restrict__ items) {
    __shared__ int s_cnt[GR_CELLS];
    __shared__ int s_part[1024];
    const long long f = blockIdx.x;
    const int t = threadIdx.x;
    const int n = counts ? min(counts[f], cap) : fixed_n;
    const orbx_keypoint *k = kps + f * cap;
    for (int c = t; c < GR_CELLS; c += 1024) s_cnt[c] = 0;
    __syncthreads();
    for (int i = t; i < n; i += 1024) {
        const int c = gr_cell_of(gp, k[i]);
        if (c >= 0) atomicAdd(&s_cnt[c], 1);
    }
    __syncthreads();
    // exclusive scan over the 3072 buckets: three per thread, Hillis-Steele over the thread sums
    const int c0 = 3 * t;
    const int a0 = s_cnt[c0], a1 = s_cnt[c0 + 1], a2 = s_cnt[c0 + 2];
    const int sum = a0 + a1 + a2;
    s_part[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = t >= o ? s_part[t - o] : 0;
        __syncthreads();
        s_part[t] += v;
        __syncthreads();
    }
    int run = s_part[t] - sum;
    int *cb = cell_begin + f * (GR_CELLS + 1);
    cb[c0] = run; s_cnt[c0] = run; run += a0;
    cb[c0 + 1] = run; s_cnt[c0 + 1] = run; run += a1;
    cb[c0 + 2] = run; s_cnt[c0 + 2] = run;
    if (t == 1023) cb[GR_CELLS] = s_part[1023];
    __syncthreads();
    uint16_t *it = items + f * cap;
    for (int i = t; i < n; i += 1024) {
        const int c = gr_cell_of(gp, k[i]);
        if (c >= 0) it[atomicAdd(&s_cnt[c], 1)] = (uint16_t)i;
    }
    __syncthreads();
    // the atomics filled every bucket in arrival order: restore feature order (buckets hold a handful of entries)
    for (int c = t; c < GR_CELLS; c += 1024) {
        const int b = cb[c], e = s_cnt[c];
        for (int i = b + 1; i < e; ++i) {
            const uint16_t v = it[i];
            int j = i - 1;
            while (j >= b && it[j] > v) { it[j + 1] = it[j]; --j; }
            it[j + 1] = v;
        }
    }
}

// One wave per query, two walks over the query's buckets: the first counts the candidates (radius / level tests only), lane 0
// then reserves that many entries of the output with one returning atomicAdd on `cursor` and records (offset, count) in
// span[query]; the second walk evaluates the Hamming distances and writes the entries in visiting order.  A reservation that
// does not fit `cap` writes nothing: the host reads the total from the cursor, grows the buffer and launches again.
__device__ __forceinline__ bool gr_pass(const DGateQuery &Q, bool check, const orbx_keypoint &kp) {
    bool pass = fabsf(kp.x - Q.x) < Q.r && fabsf(kp.y - Q.y) < Q.r;
    if (check) pass = pass && !(kp.octave < Q.min_level) && !(Q.max_level >= 0 && kp.octave > Q.max_level);
    return pass;
}
__global__ __launch_bounds__(256) void k_gate(DGrid gp, const orbx_keypoint *__restrict__ kps, const uint8_t *__restrict__ desc,
                                              const int *__restrict__ cell_begin, const uint16_t *__restrict__ items,
                                              const DGateQuery *__restrict__ q, const uint8_t *__restrict__ qdesc, int nq,
                                              uint2 *__restrict__ span, uint32_t *__restrict__ cursor,
                                              uint32_t *__restrict__ out_items, uint32_t cap, int fstride) {
    const int lane = threadIdx.x & 63;
    const int qi = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (qi >= nq) return;
    const DGateQuery Q = q[qi];
    // batched calls: target Q.frame's keypoints / descriptors / buckets are fstride records further on (item indices stay
    // relative to their target)
    kps += (long long)Q.frame * fstride;
    desc += (long long)Q.frame * fstride * 32;
    items += (long long)Q.frame * fstride;
    cell_begin += (long long)Q.frame * (GR_CELLS + 1);
    // GetFeaturesInArea's cell range (:643-668); a negative radius switches the query off
    const int x0 = max(0, (int)floorf((Q.x - gp.minx - Q.r) * gp.winv));
    const int x1 = min(GR_COLS - 1, (int)ceilf((Q.x - gp.minx + Q.r) * gp.winv));
    const int y0 = max(0, (int)floorf((Q.y - gp.miny - Q.r) * gp.hinv));
    const int y1 = min(GR_ROWS - 1, (int)ceilf((Q.y - gp.miny + Q.r) * gp.hinv));
    const bool live = Q.r >= 0.f && x0 < GR_COLS && x1 >= 0 && y0 < GR_ROWS && y1 >= 0;
    const bool check = (Q.min_level > 0) || (Q.max_level >= 0);
    int n = 0;
    if (live)
        for (int ix = x0; ix <= x1; ++ix) {
            const int b = cell_begin[ix * GR_ROWS + y0], e = cell_begin[ix * GR_ROWS + y1 + 1];
            for (int j0 = b; j0 < e; j0 += 64) {
                const int j = j0 + lane;
                const bool pass = j < e && gr_pass(Q, check, kps[items[j]]);
                n += __popcll(orbx_ballot(pass));
            }
        }
    uint32_t base = 0;
    if (lane == 0) {
        base = n > 0 ? atomicAdd(cursor, (uint32_t)n) : 0u;
        span[qi] = make_uint2(base, (uint32_t)n);
    }
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if (n == 0 || base + (uint32_t)n > cap) return;
    const uint4 *qp = (const uint4 *)(qdesc + (long long)(Q.desc >= 0 ? Q.desc : qi) * 32);
    const uint4 qa = qp[0], qb = qp[1];
    uint32_t w = base;
    for (int ix = x0; ix <= x1; ++ix) {
        const int b = cell_begin[ix * GR_ROWS + y0], e = cell_begin[ix * GR_ROWS + y1 + 1];
        for (int j0 = b; j0 < e; j0 += 64) {
            const int j = j0 + lane;
            bool pass = false;
            int i2 = 0;
            if (j < e) { i2 = items[j]; pass = gr_pass(Q, check, kps[i2]); }
            const unsigned long long m = orbx_ballot(pass);
            if (pass) {
                const uint4 *tp = (const uint4 *)(desc + (long long)i2 * 32);
                const uint4 ta = tp[0], tb = tp[1];
                const uint32_t d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                                   __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
                out_items[w + (uint32_t)orbx_wave_rank(m)] = (uint32_t)i2 | (d << 16);
            }
            w += (uint32_t)__popcll(m);
        }
    }
}

// Hamming distances of the BoW-guided policies: row r pairs descriptor rows[r].q of the first set with the features
// col_idx[col_begin .. col_begin + ncol) of the second set (the features under the same vocabulary node, in the reference's
// visiting order); distances leave as uint16 at out[out_off ..).  One wave per row.
__global__ __launch_bounds__(256) void k_block_dist(const uint8_t *__restrict__ d1, const uint8_t *__restrict__ d2,
                                                    const DDistRow *__restrict__ rows, const uint32_t *__restrict__ col_idx, int nrows,
                                                    uint16_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (r >= nrows) return;
    const DDistRow R = rows[r];
    const uint4 *qp = (const uint4 *)(d1 + (long long)R.q * 32);
    const uint4 qa = qp[0], qb = qp[1];
    for (uint32_t j = lane; j < R.ncol; j += 64) {
        const uint4 *tp = (const uint4 *)(d2 + (long long)col_idx[R.col_begin + j] * 32);
        const uint4 ta = tp[0], tb = tp[1];
        out[R.out_off + j] = (uint16_t)(__popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                                        __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w));
    }
}

// Batched SearchByBoW (orbx_search_by_bow_*_batch): the selection of src/ORBmatcher.cc:300-350 (KF <-> F, rows = keyframe
// features, columns = frame features) and :760-815 (KF <-> KF, rows = kf1 features, columns = kf2 features) for one common
// vocabulary node per wave.  With every feature index at most once per feature vector, the "already matched" test reads and
// writes only columns of this node pair, so work items are independent; inside one the rows run in the reference's order.
// Per row the lanes take the node's columns; the wave reduces 32-bit keys dist << 16 | position: the smallest is (bestDist1,
// bestIdx) with the first occurrence winning ties as the sequential `<` update does, the smallest other key bestDist2.  A
// masked column or no column at all gives 256.  Columns already matched in this node pair: a bitmap in LDS (`words` words
// per wave).  The first 64 columns stay in registers; wider nodes reload the rest per row.
#define BOW_KEY_NONE ((256u << 16) | 0xffffu)
template <bool KK>
__global__ __launch_bounds__(256) void k_bow_select(const DBowItem *__restrict__ items, int nitems, const uint32_t *__restrict__ idx,
                                                    const uint8_t *__restrict__ desc, const uint8_t *__restrict__ hmp, float nnratio,
                                                    int words, int32_t *__restrict__ out) {
    extern __shared__ uint32_t bow_taken[];
    const int lane = threadIdx.x & 63;
    const int it = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (it >= nitems) return;
    uint32_t *taken = bow_taken + (threadIdx.x >> 6) * words;
    const DBowItem I = items[it];
    for (uint32_t w = lane; w < (I.ncol + 31) / 32; w += 64) taken[w] = 0;
    uint32_t cidx0 = 0;
    bool cok0 = false;
    uint4 ca = make_uint4(0, 0, 0, 0), cb = ca;
    if ((uint32_t)lane < I.ncol) {
        cidx0 = idx[I.cbeg + lane];
        cok0 = !KK || hmp[I.cbase + cidx0];
        const uint4 *p = (const uint4 *)(desc + (size_t)(I.cbase + cidx0) * 32);
        ca = p[0]; cb = p[1];
    }
    for (uint32_t r0 = 0; r0 < I.nrow; r0 += 64) {
        // the next 64 rows: index, MapPoint flag and descriptor one per lane, broadcast row by row with readlane
        uint32_t ridx = 0;
        int rok = 0;
        uint4 ra = make_uint4(0, 0, 0, 0), rb = ra;
        if (r0 + lane < I.nrow) {
            ridx = idx[I.rbeg + r0 + lane];
            rok = hmp[I.rbase + ridx];
            if (rok) { const uint4 *p = (const uint4 *)(desc + (size_t)(I.rbase + ridx) * 32); ra = p[0]; rb = p[1]; }
        }
        const uint32_t nr = min(64u, I.nrow - r0);
        for (uint32_t rr = 0; rr < nr; ++rr) {
            if (!__builtin_amdgcn_readlane(rok, rr)) continue;                       // no MapPoint in the row's keyframe
            const uint4 qa = make_uint4(__builtin_amdgcn_readlane(ra.x, rr), __builtin_amdgcn_readlane(ra.y, rr),
                                        __builtin_amdgcn_readlane(ra.z, rr), __builtin_amdgcn_readlane(ra.w, rr));
            const uint4 qb = make_uint4(__builtin_amdgcn_readlane(rb.x, rr), __builtin_amdgcn_readlane(rb.y, rr),
                                        __builtin_amdgcn_readlane(rb.z, rr), __builtin_amdgcn_readlane(rb.w, rr));
            uint32_t b1 = BOW_KEY_NONE, b2 = BOW_KEY_NONE;
            for (uint32_t c0 = 0; c0 < I.ncol; c0 += 64) {
                const uint32_t c = c0 + lane;
                uint32_t key = BOW_KEY_NONE;
                if (c < I.ncol && !((taken[c >> 5] >> (c & 31)) & 1u)) {
                    uint4 ta = ca, tb = cb;
                    bool ok = cok0;
                    if (c0 > 0) {
                        const uint32_t ic = idx[I.cbeg + c];
                        ok = !KK || hmp[I.cbase + ic];
                        if (ok) { const uint4 *p = (const uint4 *)(desc + (size_t)(I.cbase + ic) * 32); ta = p[0]; tb = p[1]; }
                    }
                    if (ok) {
                        const uint32_t d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                                           __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
                        key = (d << 16) | c;
                    }
                }
                if (key < b1) { b2 = b1; b1 = key; }
                else if (key < b2) b2 = key;
            }
            const uint32_t m1 = orbx_wave_min(b1);
            const uint32_t m2 = orbx_wave_min(b1 == m1 ? b2 : b1);
            const int d1 = (int)(m1 >> 16), d2 = (int)(m2 >> 16);
            if ((KK ? d1 < 50 : d1 <= 50) && (float)d1 < nnratio * (float)d2) {   // TH_LOW: '<' in KF <-> KF (:809), '<=' (:339)
                const uint32_t c = m1 & 0xffffu;
                const uint32_t irow = (uint32_t)__builtin_amdgcn_readlane((int)ridx, rr);
                const uint32_t icol = c < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)cidx0, c) : idx[I.cbeg + c];
                if (lane == 0) {
                    taken[c >> 5] |= 1u << (c & 31);
                    if (KK) out[I.obase + irow] = (int32_t)icol;
                    else out[I.obase + icol] = (int32_t)irow;
                }
            }
        }
    }
}

// bin of RotHist::push (orbx_policies.cpp, src/ORBmatcher.cc:340-351), -1 = the reference's `bin >= 0 && bin < HISTO` fails
__device__ __forceinline__ int bow_rot_bin(float a1, float a2) {
    float rot = a1 - a2;
    if (rot < 0.0f) rot += 360.0f;
    const float r = roundf(rot * (30 / 360.0f));
    if (!(r >= 0.0f && r <= 30.0f)) return -1;
    const int bin = (int)r;
    return bin == 30 ? 0 : bin;
}
// Rotation check (ComputeThreeMaxima + the removal loop, :380-398) and the match count: one workgroup per problem.  It depends
// on the set of matches in each bin only, so it runs after all of the problem's node pairs.  1024 threads: one pass over a
// 1000-feature output (the kernel is a chain of dependent loads; a 256-thread version took 9 us).
#define BOW_ROT_THREADS 1024
template <bool KK>
__global__ __launch_bounds__(BOW_ROT_THREADS) void k_bow_rot(int nout, const uint32_t *__restrict__ cand_base, const float *__restrict__ ang,
                                                 int check, int32_t *__restrict__ out, int32_t *__restrict__ counts) {
    __shared__ int hist[30];
    __shared__ int keep[3];
    __shared__ int total;
    const int k = blockIdx.x, t = threadIdx.x;
    int32_t *o = out + (size_t)k * nout;
    const uint32_t base = cand_base[k];
    if (t < 30) hist[t] = 0;
    if (t == 0) total = 0;
    __syncthreads();
    if (check) {
        for (int i = t; i < nout; i += BOW_ROT_THREADS) {
            const int m = o[i];
            if (m < 0) continue;
            const int b = KK ? bow_rot_bin(ang[i], ang[base + m]) : bow_rot_bin(ang[base + m], ang[i]);
            if (b >= 0) atomicAdd(&hist[b], 1);
        }
        __syncthreads();
        if (t == 0) {   // orbx_three_maxima
            int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
            for (int i = 0; i < 30; ++i) {
                const int s = hist[i];
                if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
                else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
                else if (s > max3) { max3 = s; i3 = i; }
            }
            if (max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
            else if (max3 < 0.1f * (float)max1) { i3 = -1; }
            keep[0] = i1; keep[1] = i2; keep[2] = i3;
        }
        __syncthreads();
    }
    int n = 0;
    for (int i = t; i < nout; i += BOW_ROT_THREADS) {
        const int m = o[i];
        if (m < 0) continue;
        if (check) {
            const int b = KK ? bow_rot_bin(ang[i], ang[base + m]) : bow_rot_bin(ang[base + m], ang[i]);
            if (b >= 0 && b != keep[0] && b != keep[1] && b != keep[2]) { o[i] = -1; continue; }
        }
        ++n;
    }
    const int s = orbx_wave_sum(n);
    if ((t & 63) == 0) atomicAdd(&total, s);
    __syncthreads();
    if (t == 0) counts[k] = total;
}

// ------------------------------------------------------------------------------------------------
// K12: the two tracking matchers, batched and device-resident (orbx_track.h): SearchByProjection(CurrentFrame, LastFrame, th,
// bMono) (reference src/ORBmatcher.cc:1702-1871) and SearchByProjection(F, vpMapPoints, th) (:69-184) for many (frame, point
// set) problems in one call.  The current frames are the device batch buffers and the grids of k_grid_build.
//   k_track_project (frame policy): one thread per last-frame point, the projection of :1742-1783 in the arithmetic of
//     orbx_search_by_projection_frame; the packed record becomes the GetFeaturesInArea query in place.
//   k_track_cand: one wave per point walks the query's buckets in k_gate's order and keeps, instead of a candidate list, the
//     smallest key dist << 16 | visiting position (the two smallest for the map-point policy) over the candidates that pass
//     the tests that do not depend on the selection state: window, level band, u_right gate.
//   k_track_select: one wave per problem takes the points in order with the blocked features (assigned to a point with
//     Observations() > 0) as a bitmap in LDS.  Removing candidates cannot change the smallest keys among the others, so a
//     point whose stored candidates are all unblocked at its turn has the reference's result; otherwise the wave walks that
//     point's buckets again with the blocked test.  Frame policy: the rotation check over the accept events follows.
// ------------------------------------------------------------------------------------------------
#define TRK_NONE 0xffffffffu
#define TRK_TH_HIGH 100u
struct TrackBest { uint32_t k1, p1, k2, p2; };   // key, payload (feature index | octave << 16) of the best and the second
// the walk of k_gate over the buckets of Q's window in frame (kps, desc, ur, cb, items; n features): every lane keeps its
// smallest keys, the wave reduces them (keys are unique: the visiting position is).  blocked != nullptr: features whose bit is
// set do not count.  All 64 lanes must be active.
template <bool TWO>
__device__ __forceinline__ TrackBest track_scan(const DGrid &gp, const DTrackQ &Q, const uint4 qa, const uint4 qb,
                                                const orbx_keypoint *__restrict__ kps, const uint8_t *__restrict__ desc,
                                                const float *__restrict__ ur, const int *__restrict__ cb,
                                                const uint16_t *__restrict__ items, int n, const uint32_t *blocked, int lane) {
    const int x0 = max(0, (int)floorf((Q.x - gp.minx - Q.r) * gp.winv));
    const int x1 = min(GR_COLS - 1, (int)ceilf((Q.x - gp.minx + Q.r) * gp.winv));
    const int y0 = max(0, (int)floorf((Q.y - gp.miny - Q.r) * gp.hinv));
    const int y1 = min(GR_ROWS - 1, (int)ceilf((Q.y - gp.miny + Q.r) * gp.hinv));
    const bool live = Q.r >= 0.f && x0 < GR_COLS && x1 >= 0 && y0 < GR_ROWS && y1 >= 0;
    const bool check = (Q.min_level > 0) || (Q.max_level >= 0);
    uint32_t b1 = TRK_NONE, b2 = TRK_NONE, pay1 = 0, pay2 = 0;
    if (live) {
        int pos = 0;
        for (int ix = x0; ix <= x1; ++ix) {
            // a grid that does not belong to these buffers must not lead outside them
            const int b = max(cb[ix * GR_ROWS + y0], 0), e = min(cb[ix * GR_ROWS + y1 + 1], n);
            for (int j0 = b; j0 < e; j0 += 64) {
                const int j = j0 + lane;
                if (j < e) {
                    const int i2 = items[j];
                    if (i2 < n) {
                        const orbx_keypoint *kp = kps + i2;
                        const int oct = kp->octave;
                        bool pass = fabsf(kp->x - Q.x) < Q.r && fabsf(kp->y - Q.y) < Q.r;
                        if (check) pass = pass && !(oct < Q.min_level) && !(Q.max_level >= 0 && oct > Q.max_level);
                        if (pass && blocked) pass = !((blocked[i2 >> 5] >> (i2 & 31)) & 1u);
                        if (pass && ur) {
                            const float u2 = ur[i2];
                            if (u2 > 0 && fabsf(Q.ur - u2) > Q.r) pass = false;
                        }
                        if (pass) {
                            const uint4 *tp = (const uint4 *)(desc + (long long)i2 * 32);
                            const uint4 ta = tp[0], tb = tp[1];
                            const uint32_t d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                                               __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
                            const uint32_t key = (d << 16) | (uint32_t)(pos + (j - b)), pay = (uint32_t)i2 | ((uint32_t)(oct & 0xff) << 16);
                            if (key < b1) { b2 = b1; pay2 = pay1; b1 = key; pay1 = pay; }
                            else if (TWO && key < b2) { b2 = key; pay2 = pay; }
                        }
                    }
                }
            }
            pos += e > b ? e - b : 0;
        }
    }
    TrackBest R;
    R.k1 = orbx_wave_min(b1);
    const bool own1 = b1 == R.k1 && R.k1 != TRK_NONE;
    R.p1 = orbx_wave_min(own1 ? pay1 : TRK_NONE);
    R.k2 = TRK_NONE; R.p2 = TRK_NONE;
    if (TWO) {
        const uint32_t c = own1 ? b2 : b1, cp = own1 ? pay2 : pay1;
        R.k2 = orbx_wave_min(c);
        R.p2 = orbx_wave_min(c == R.k2 && R.k2 != TRK_NONE ? cp : TRK_NONE);
    }
    return R;
}

struct DTrackCam { float fx, fy, cx, cy, minx, maxx, miny, maxy, mbf; int fma_mode; };
// one row of Rcw * x + tcw: cv::gemm's 3x3 * 3x1 float special case (oracle/orb_oracle_match.c: gemm3)
__device__ __forceinline__ float track_gemm3(const float *a, const float *b, float c) {
    const float t = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    return (float)((double)t * 1.0 + (double)c * 1.0);
}
__global__ __launch_bounds__(256) void k_track_project(DTrackCam cam, const DTrackProb *__restrict__ probs, DTrackQ *__restrict__ q,
                                                       int nq) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    DTrackQ Q = q[i];
    if (!(Q.r >= 0.f)) return;
    const DTrackProb P = probs[Q.prob];
    const float w[3] = {Q.x, Q.y, Q.ur};
    float pc[3];
    for (int r = 0; r < 3; ++r) pc[r] = track_gemm3(&P.Rcw[3 * r], w, P.tcw[r]);
    const float invzc = (float)(1.0 / (double)pc[2]);
    bool ok = !(invzc < 0);
    float u = 0.f, v = 0.f, ur = 0.f;
    if (ok) {
        if (cam.fma_mode) { u = __builtin_fmaf(cam.fx * pc[0], invzc, cam.cx); v = __builtin_fmaf(cam.fy * pc[1], invzc, cam.cy); }
        else { u = cam.fx * pc[0] * invzc + cam.cx; v = cam.fy * pc[1] * invzc + cam.cy; }
        ok = !(u < cam.minx || u > cam.maxx || v < cam.miny || v > cam.maxy);
        ur = cam.fma_mode ? __builtin_fmaf(-cam.mbf, invzc, u) : u - cam.mbf * invzc;
    }
    const int oct = Q.min_level;
    if (!ok) { Q.r = -1.0f; Q.min_level = Q.max_level = -1; }
    else if (P.dir == 1) { Q.min_level = oct; Q.max_level = -1; }
    else if (P.dir == 2) { Q.min_level = 0; Q.max_level = oct; }
    else { Q.min_level = oct - 1; Q.max_level = oct + 1; }
    Q.x = u; Q.y = v; Q.ur = ur;
    q[i] = Q;
}

// Frame::isInFrustum (src/Frame.cc:529-620) + MapPoint::PredictScale (src/MapPoint.cc:706-721) + the first lines of
// SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:82-101, RadiusByViewingCos :187-194) for the local-map policy: one
// thread per (problem, point) -- blockIdx.y = the problem (from prob0 on), blockIdx.x * 256 + threadIdx.x = the point in its list
// -- turns a pool point under the problem's pose into the query k_track_cand / k_track_select read, or switches it off
// (r = -1), and gathers the point's descriptor from the pool.  Every expression in the reference's order and arithmetic; the
// level comes from the threshold table (orbx_predict_scale_table), which travels with the scale factors in the argument struct.
struct DTrackFrustumArgs {
    DTrackCam cam;
    int nlevels;
    float thr[ORBX_PS_LEVELS], scale[ORBX_PS_LEVELS];
};
__global__ __launch_bounds__(256) void k_track_frustum(DTrackFrustumArgs A, int prob0, const DTrackProb *__restrict__ probs,
                                                       const DTrackLocal *__restrict__ locals, const DTrackPoolPt *__restrict__ pool,
                                                       const uint8_t *__restrict__ pdesc, const int32_t *__restrict__ index,
                                                       const uint8_t *__restrict__ skip, DTrackQ *__restrict__ q,
                                                       uint8_t *__restrict__ qdesc, uint8_t *__restrict__ in_view,
                                                       orbx_track_state *__restrict__ track) {
    const int k = prob0 + blockIdx.y;
    const DTrackProb P = probs[k];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.nq) return;
    const long long g = (long long)P.q_begin + i;
    const DTrackLocal E = locals[k];
    const DTrackCam &cam = A.cam;
    const int pi = index[g];
    const DTrackPoolPt T = pool[pi];
    bool ok = !skip[g];
    float u = 0.f, v = 0.f, ur = 0.f, viewCos = 0.f, r = -1.0f;
    int level = 0;
    if (ok) {
        float pc[3];
        for (int rr = 0; rr < 3; ++rr) pc[rr] = track_gemm3(&P.Rcw[3 * rr], T.P, P.tcw[rr]);
        ok = !(pc[2] < 0.0f);
        const float invz = 1.0f / pc[2];
        if (cam.fma_mode) { u = __builtin_fmaf(cam.fx * pc[0], invz, cam.cx); v = __builtin_fmaf(cam.fy * pc[1], invz, cam.cy); }
        else { u = cam.fx * pc[0] * invz + cam.cx; v = cam.fy * pc[1] * invz + cam.cy; }
        ok = ok && !(u < cam.minx || u > cam.maxx) && !(v < cam.miny || v > cam.maxy);
        const float maxDistance = 1.2f * T.dmax, minDistance = 0.8f * T.dmin;
        const float po[3] = {T.P[0] - E.Ow[0], T.P[1] - E.Ow[1], T.P[2] - E.Ow[2]};
        double s2 = 0.0, dot = 0.0;   // cv::norm, Mat::dot: double sums in element order (the products of floats are exact)
        for (int c = 0; c < 3; ++c) { s2 += (double)po[c] * (double)po[c]; dot += (double)po[c] * (double)T.Pn[c]; }
        const float dist = (float)sqrt(s2);
        ok = ok && !(dist < minDistance || dist > maxDistance);
        viewCos = (float)(dot / (double)dist);
        ok = ok && !(viewCos < E.cos_limit);
        const float ratio = T.dmax / dist;
#pragma unroll
        for (int l = 1; l < ORBX_PS_LEVELS; ++l) level += (l < A.nlevels && ratio >= A.thr[l]) ? 1 : 0;
        ur = cam.fma_mode ? __builtin_fmaf(-cam.mbf, invz, u) : u - cam.mbf * invz;
        r = (double)viewCos > 0.998 ? 2.5f : 4.0f;
        if ((double)E.th != 1.0) r *= E.th;
        float sc = A.scale[0];
#pragma unroll
        for (int l = 1; l < ORBX_PS_LEVELS; ++l) sc = level == l ? A.scale[l] : sc;   // selects: the table stays in registers
        r *= sc;
    }
    DTrackQ Q;
    Q.x = ok ? u : 0.f; Q.y = ok ? v : 0.f; Q.ur = ok ? ur : 0.f;
    Q.r = ok ? r : -1.0f;
    Q.min_level = ok ? level - 1 : -1; Q.max_level = ok ? level : -1;
    Q.obs = T.obs; Q.angle = 0.f; Q.prob = k; Q.pad = 0;
    q[g] = Q;
    if (ok) {
        const uint4 *sp = (const uint4 *)(pdesc + (long long)pi * 32);
        uint4 *dp = (uint4 *)(qdesc + g * 32);
        dp[0] = sp[0]; dp[1] = sp[1];
        if (track) { orbx_track_state S; S.proj_x = u; S.proj_y = v; S.proj_xr = ur; S.view_cos = viewCos; S.level = level; track[g] = S; }
    }
    if (in_view) in_view[g] = ok ? 1 : 0;
}

template <bool TWO>
__global__ __launch_bounds__(256) void k_track_cand(DGrid gp, const DTrackProb *__restrict__ probs, const DTrackQ *__restrict__ q,
                                                    const uint8_t *__restrict__ qdesc, int nq, const orbx_keypoint *__restrict__ kps,
                                                    const uint8_t *__restrict__ desc, const float *__restrict__ ur,
                                                    const int *__restrict__ counts, int cap, const int *__restrict__ cell_begin,
                                                    const uint16_t *__restrict__ items, uint4 *__restrict__ cand) {
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (g >= nq) return;
    const DTrackQ Q = q[g];
    TrackBest B = {TRK_NONE, TRK_NONE, TRK_NONE, TRK_NONE};
    if (Q.r >= 0.f) {
        const long long f = probs[Q.prob].frame;
        const int n = min(counts[f], cap);
        const uint4 *qp = (const uint4 *)(qdesc + (long long)g * 32);
        B = track_scan<TWO>(gp, Q, qp[0], qp[1], kps + f * cap, desc + f * cap * 32, ur ? ur + f * cap : nullptr,
                            cell_begin + f * (GR_CELLS + 1), items + f * cap, n, nullptr, lane);
    }
    if (lane == 0) cand[g] = make_uint4(B.k1, B.p1, B.k2, B.p2);
}

// One wave per problem.  Dynamic LDS: the blocked bitmap (`words` words, >= ceil(cap / 32)) | the 30 bins of the histogram.
// MP = the map-point policy (two stored candidates, level-aware ratio test, bitmap seeded from frame_observations).
template <bool MP>
__global__ __launch_bounds__(64) void k_track_select(DGrid gp, const DTrackProb *__restrict__ probs, const DTrackQ *__restrict__ q,
                                                     const uint8_t *__restrict__ qdesc, const uint4 *__restrict__ cand,
                                                     const uint32_t *__restrict__ seed, int words,
                                                     const orbx_keypoint *__restrict__ kps, const uint8_t *__restrict__ desc,
                                                     const float *__restrict__ ur, const int *__restrict__ counts, int cap,
                                                     const int *__restrict__ cell_begin, const uint16_t *__restrict__ items,
                                                     float nnratio, int check, int32_t *__restrict__ ev, int32_t *__restrict__ out,
                                                     int32_t *__restrict__ nmatches) {
    extern __shared__ uint32_t trk_lds[];
    uint32_t *blocked = trk_lds;
    int *hist = (int *)(trk_lds + words);
    const int lane = threadIdx.x;
    const int k = blockIdx.x;
    const DTrackProb P = probs[k];
    const long long f = P.frame;
    const int n = min(counts[f], cap);
    kps += f * cap; desc += f * cap * 32; items += f * cap; cell_begin += f * (GR_CELLS + 1);
    if (ur) ur += f * cap;
    int32_t *o = out + (long long)k * cap;
    q += P.q_begin; qdesc += (long long)P.q_begin * 32; cand += P.q_begin; ev += P.q_begin;
    for (int w = lane; w < words; w += 64) blocked[w] = MP ? seed[(long long)k * words + w] : 0u;
    for (int i = lane; i < n; i += 64) o[i] = -1;
    if (lane < 30) hist[lane] = 0;
    __syncthreads();
    int total = 0;
    for (int p0 = 0; p0 < P.nq; p0 += 64) {
        uint4 c = make_uint4(TRK_NONE, TRK_NONE, TRK_NONE, TRK_NONE);
        int obsv = 0;
        if (p0 + lane < P.nq) { c = cand[p0 + lane]; obsv = q[p0 + lane].obs; }
        int evv = -1;
        const int nb = min(64, P.nq - p0);
        for (int rr = 0; rr < nb; ++rr) {
            uint32_t k1 = (uint32_t)__builtin_amdgcn_readlane((int)c.x, rr);
            if ((k1 >> 16) > TRK_TH_HIGH) continue;   // no candidate, or none within TH_HIGH: a second walk cannot find a closer one
            uint32_t p1 = (uint32_t)__builtin_amdgcn_readlane((int)c.y, rr), k2 = TRK_NONE, p2 = TRK_NONE;
            const uint32_t i1 = p1 & 0xffffu;
            uint32_t hit = (blocked[i1 >> 5] >> (i1 & 31)) & 1u;
            if (MP) {
                k2 = (uint32_t)__builtin_amdgcn_readlane((int)c.z, rr);
                p2 = (uint32_t)__builtin_amdgcn_readlane((int)c.w, rr);
                if (k2 != TRK_NONE) { const uint32_t i2 = p2 & 0xffffu; hit |= (blocked[i2 >> 5] >> (i2 & 31)) & 1u; }
            }
            if (__builtin_amdgcn_readfirstlane((int)hit)) {   // the same in every lane: the branch stays scalar
                const uint4 *qp = (const uint4 *)(qdesc + (long long)(p0 + rr) * 32);
                const TrackBest B = track_scan<MP>(gp, q[p0 + rr], qp[0], qp[1], kps, desc, ur, cell_begin, items, n, blocked, lane);
                k1 = B.k1; p1 = B.p1; k2 = B.k2; p2 = B.p2;
                if ((k1 >> 16) > TRK_TH_HIGH) continue;
            }
            if (MP) {
                const int l1 = (int)((p1 >> 16) & 0xffu), l2 = k2 == TRK_NONE ? -1 : (int)((p2 >> 16) & 0xffu);
                const int d1 = (int)(k1 >> 16), d2 = k2 == TRK_NONE ? 256 : (int)(k2 >> 16);
                if (l1 == l2 && (float)d1 > nnratio * (float)d2) continue;
            }
            const uint32_t idx = p1 & 0xffffu;
            if (lane == 0) o[idx] = p0 + rr;
            // every lane writes the (same) word: each then reads its own store back in the next test
            if (__builtin_amdgcn_readlane(obsv, rr) > 0) blocked[idx >> 5] |= 1u << (idx & 31);
            if (lane == rr) evv = (int)idx;
            ++total;
        }
        if (!MP && p0 + lane < P.nq) ev[p0 + lane] = evv;
    }
    if (MP) {
        if (lane == 0) nmatches[k] = total;
        return;
    }
    // the rotation check over the accept events (src/ORBmatcher.cc:1842-1868): an event in a dropped bin takes the feature's
    // match away and one off the count, also where a later event had taken the feature over
    int dropped = 0;
    if (check) {
        __syncthreads();   // the events and the assignments written above
        for (int i = lane; i < P.nq; i += 64) {
            const int i2 = ev[i];
            if (i2 < 0) continue;
            const int b = bow_rot_bin(q[i].angle, kps[i2].angle);
            if (b >= 0) atomicAdd(&hist[b], 1);
        }
        __syncthreads();
        int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;   // orbx_three_maxima
        for (int i = 0; i < 30; ++i) {
            const int s = hist[i];
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
            else if (s > max3) { max3 = s; i3 = i; }
        }
        if (max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
        else if (max3 < 0.1f * (float)max1) { i3 = -1; }
        for (int i = lane; i < P.nq; i += 64) {
            const int j = ev[i];
            if (j < 0) continue;
            const int b = bow_rot_bin(q[i].angle, kps[j].angle);
            if (b >= 0 && b != i1 && b != i2 && b != i3) { o[j] = -1; ++dropped; }
        }
    }
    const int nd = orbx_wave_sum(dropped);
    if (lane == 0) nmatches[k] = total - nd;
}

__global__ void k_clear(int *a, int na, int *b, int nb, int *c, int nc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < na) a[i] = 0;
    if (b && i < nb) b[i] = 0;
    if (c && i < nc) c[i] = 0;
}

// ------------------------------------------------------------------------------------------------
// K14: keyframe database (orbx_kfdb.cpp): steps 1-3 of KeyFrameDatabase::DetectRelocalizationCandidates / DetectLoopCandidates
// (reference src/KeyFrameDatabase.cc:114-411) and DBoW2's scoring functions (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp).
// An entry is a slot (offset, length) into the pooled BowVectors: words ascending, values next to them.
// ------------------------------------------------------------------------------------------------
#define KF_BATCH 32   // records a wave collects in LDS before it appends them
// index of `w` in the ascending array `a[0..n)`, -1 if absent
template <class P> __device__ __forceinline__ int kf_find(P a, int n, uint32_t w) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < w) lo = mid + 1; else hi = mid;
    }
    return lo < n && a[lo] == w ? lo : -1;
}
// One wave per (query, entry): lanes stride over the entry's words and test membership in the query's; ballot / popcount
// gives mn*Words, the wave minimum the smallest common word (the entry's position key in lKFsSharingWords).  Integer only.
template <class P> __device__ __forceinline__ void kf_common_entries(P qw, int nq, uint32_t q, const uint2 *__restrict__ slots,
                                                                     int nslots, const uint32_t *__restrict__ pool_w,
                                                                     const uint8_t *__restrict__ connected, int *__restrict__ qmax,
                                                                     uint32_t *__restrict__ cursor, DKfRec *__restrict__ rec,
                                                                     uint32_t cap, DKfRec *s_rec) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // Records are collected per wave and appended KF_BATCH at a time, the maximum is kept per wave: one atomic on the shared
    // cursor per sharer serialised the whole grid on one address (measured: 4.6 ms of a 4.8 ms launch).
    int nbuf = 0, wmax = 0;
    auto flush = [&]() {
        orbx_wave_sync();
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(cursor, (uint32_t)nbuf);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        for (int k = lane; k < nbuf; k += 64)
            if (base + k < cap) rec[base + k] = s_rec[k];
        orbx_wave_sync();
        nbuf = 0;
    };
    for (int e = blockIdx.x * 4 + wave; e < nslots; e += gridDim.x * 4) {
        const uint2 s = slots[e];
        int cnt = 0;
        uint32_t minw = 0xffffffffu;
        // Four words per lane and round: the loads are issued together and the four searches advance in lockstep (the trip
        // count depends on nq alone), so four independent chains hide the latency of one.
        for (uint32_t i0 = 0; i0 < s.y; i0 += 256) {
            uint32_t w[4], base[4];
            bool in[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t i = i0 + 64 * k + lane;
                in[k] = i < s.y;
                w[k] = in[k] ? pool_w[s.x + i] : 0u;
                base[k] = 0;
            }
            // if w is in qw[0..nq) its index stays inside [base, base + len)
            for (int len = nq; len > 1;) {
                const int half = len >> 1;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (qw[base[k] + half - 1] < w[k]) base[k] += half;
                len -= half;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool f = in[k] && qw[base[k]] == w[k];
                if (f) minw = min(minw, w[k]);
                cnt += __popcll(orbx_ballot(f));
            }
        }
        if (cnt == 0) continue;                      // wave-uniform
        minw = orbx_wave_min(minw);
        const uint32_t conn = connected && connected[e] ? ORBX_KF_CONNECTED : 0u;
        if (!conn) wmax = max(wmax, cnt);            // maxCommonWords runs over lKFsSharingWords only
        if (lane == 0) {
            DKfRec R;
            R.q = q; R.slot = (uint32_t)e; R.count = (uint32_t)cnt; R.minword = minw; R.flags = conn; R.score = 0.0f;
            s_rec[nbuf] = R;
        }
        if (++nbuf == KF_BATCH) flush();
    }
    if (nbuf) flush();
    if (wmax && lane == 0) atomicMax(&qmax[q], wmax);
}
// grid (entry groups, queries).  The query's sorted word ids are staged in LDS when they fit (the usual BowVector has at most
// one word per feature); a longer query is searched where it lies: it is read by every wave of the grid row, so it stays in
// L2, and the search is the same code -- a rare case is not worth a second LDS budget that would halve the occupancy of the
// common one.
__global__ __launch_bounds__(256) void k_kfdb_common(const uint2 *__restrict__ slots, int nslots, const uint32_t *__restrict__ pool_w,
                                                     const uint32_t *__restrict__ qw_all, const int *__restrict__ q_begin, int q0,
                                                     const uint8_t *__restrict__ connected, int *__restrict__ qmax,
                                                     uint32_t *__restrict__ cursor, DKfRec *__restrict__ rec, uint32_t cap) {
    __shared__ uint32_t s_q[ORBX_KFDB_LDS_WORDS];
    __shared__ DKfRec s_rec[4][KF_BATCH];
    DKfRec *my_rec = s_rec[threadIdx.x >> 6];
    const int q = q0 + blockIdx.y;
    const int qb = q_begin[q], nq = q_begin[q + 1] - qb;
    if (nq <= 0) return;
    if (nq <= ORBX_KFDB_LDS_WORDS) {
        for (int i = threadIdx.x; i < nq; i += 256) s_q[i] = qw_all[qb + i];
        __syncthreads();
        kf_common_entries((const uint32_t *)s_q, nq, (uint32_t)q, slots, nslots, pool_w, connected, qmax, cursor, rec, cap, my_rec);
    } else {
        kf_common_entries(qw_all + qb, nq, (uint32_t)q, slots, nslots, pool_w, connected, qmax, cursor, rec, cap, my_rec);
    }
}
// TemplatedVocabulary::score(v1 = query, v2 = entry) by one wave.  The lanes find the common words and compute the per-word
// terms in parallel; the terms are compacted IN WORD ORDER into LDS and lane 0 adds them one after the other in double, as the
// reference's merge walk does (floating-point addition is not associative: no tree, no reassociation).  L2 / dot product
// under ORBX_FP_GCC_FMA keep both factors so that lane 0 performs the fused multiply-add GCC contracts `score += vi * wi` into.
// The result is valid on lane 0.  KL (needs libm's log) is not computed here.
__device__ __forceinline__ double kf_score_wave(const uint32_t *__restrict__ qw, const double *__restrict__ qv, int nq,
                                                const uint32_t *__restrict__ ew, const double *__restrict__ ev, int ne,
                                                int scoring, bool fma_mode, double *s_a, double *s_b) {
    const int lane = threadIdx.x & 63;
    const bool fused = fma_mode && (scoring == 1 || scoring == 5);
    double acc = 0.0;
    for (int i0 = 0; i0 < ne; i0 += 64) {
        const int i = i0 + lane;
        bool f = false;
        double a = 0.0, b = 0.0;
        if (i < ne) {
            const int j = kf_find(qw, nq, ew[i]);
            if (j >= 0) {
                const double vi = qv[j], wi = ev[i];
                f = true;
                if (scoring == 0) a = fabs(vi - wi) - fabs(vi) - fabs(wi);
                else if (scoring == 2) { if (vi + wi != 0.0) a = vi * wi / (vi + wi); else f = false; }
                else if (scoring == 4) a = sqrt(vi * wi);
                else if (fused) { a = vi; b = wi; }
                else a = vi * wi;
            }
        }
        const unsigned long long bal = orbx_ballot(f);
        if (f) {
            const int r = orbx_wave_rank(bal);
            s_a[r] = a;
            if (fused) s_b[r] = b;
        }
        orbx_wave_sync();
        if (lane == 0) {
            const int n = __popcll(bal);
            if (fused) for (int k = 0; k < n; ++k) acc = __builtin_fma(s_a[k], s_b[k], acc);
            else for (int k = 0; k < n; ++k) acc = acc + s_a[k];
        }
        orbx_wave_sync();
    }
    if (scoring == 0) return -acc / 2.0;
    if (scoring == 1) return acc >= 1 ? 1.0 : 1.0 - sqrt(1.0 - acc);
    if (scoring == 2) return 2. * acc;
    return acc;
}
// step 3: one wave per record whose entry is listed and has more than minCommonWords = maxCommonWords * 0.8f common words
__global__ __launch_bounds__(256) void k_kfdb_score(DKfRec *__restrict__ rec, const uint32_t *__restrict__ cursor, uint32_t cap,
                                                    const int *__restrict__ qmax, const uint2 *__restrict__ slots,
                                                    const uint32_t *__restrict__ pool_w, const double *__restrict__ pool_v,
                                                    const uint32_t *__restrict__ qw_all, const double *__restrict__ qv_all,
                                                    const int *__restrict__ q_begin, int scoring, int fma_mode) {
    __shared__ double s_terms[4][2][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n = min(*cursor, cap);
    for (uint32_t r = blockIdx.x * 4 + wave; r < n; r += gridDim.x * 4) {
        const DKfRec R = rec[r];
        if (R.flags & ORBX_KF_CONNECTED) continue;
        const int min_common = (int)((float)qmax[R.q] * 0.8f);
        if ((int)R.count <= min_common) continue;
        const uint2 s = slots[R.slot];
        const int qb = q_begin[R.q];
        const double sc = kf_score_wave(qw_all + qb, qv_all + qb, q_begin[R.q + 1] - qb, pool_w + s.x, pool_v + s.x, (int)s.y,
                                        scoring, fma_mode != 0, s_terms[wave][0], s_terms[wave][1]);
        if (lane == 0) {
            rec[r].score = (float)sc;               // `float si = mpVoc->score(...)`: the double narrowed once
            rec[r].flags = R.flags | ORBX_KF_SCORED;
        }
    }
}
// plain score calls against named entries (the minScore loop of LoopClosing::DetectLoop): one wave per entry, one query
__global__ __launch_bounds__(256) void k_kfdb_score_slots(const uint32_t *__restrict__ slot_list, int n, const uint2 *__restrict__ slots,
                                                          const uint32_t *__restrict__ pool_w, const double *__restrict__ pool_v,
                                                          const uint32_t *__restrict__ qw, const double *__restrict__ qv, int nq,
                                                          int scoring, int fma_mode, double *__restrict__ out) {
    __shared__ double s_terms[4][2][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int k = blockIdx.x * 4 + wave; k < n; k += gridDim.x * 4) {
        const uint2 s = slots[slot_list[k]];
        const double sc = kf_score_wave(qw, qv, nq, pool_w + s.x, pool_v + s.x, (int)s.y, scoring, fma_mode != 0,
                                        s_terms[wave][0], s_terms[wave][1]);
        if (lane == 0) out[k] = sc;
    }
}

// ------------------------------------------------------------------------------------------------
// MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth over a ragged batch of points (orbx_mappoint.h)
// ------------------------------------------------------------------------------------------------
#include "orbx_mappoint.h"
// rows: obs_row == nullptr: row t is desc + 32 t (the uploaded block); otherwise desc is the caller's pool and row t is
// desc + 32 obs_row[t].  Either way 16-byte aligned.
struct DMpDistinct {
    const int32_t *obs_begin; const uint8_t *desc; const int64_t *obs_row;
    const int32_t *order; int count;          // the points of this launch
    int32_t *best_idx, *best_median; uint4 *best_desc;
};
__device__ __forceinline__ const uint4 *mp_row(const DMpDistinct &A, long long t) {
    return (const uint4 *)(A.desc + 32 * (A.obs_row ? (long long)A.obs_row[t] : t));
}
__device__ __forceinline__ uint32_t mp_dist(const uint4 &qa, const uint4 &qb, const uint4 &ta, const uint4 &tb) {
    return __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
           __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
}
// N <= ORBX_MP_GROUP = 16: a group of 16 lanes serves a point, four points per wave.  Lane i owns row i of D: its descriptor
// in registers, the others broadcast from LDS, the row packed two distances per register (0xffff beyond N, above every
// threshold).  Distances are at most 256, so the median needs no sort: it is the smallest v with count(D[i][.] <= v) >=
// (N - 1) / 2 + 1, found in nine bisection steps over [0, 256].  BestIdx = the group minimum of median << 22 | i: the first of
// equal medians wins, as the reference's strict `<` has it.  Every lane runs to the end (the row reduction wants whole rows).
__global__ __launch_bounds__(256) void k_mp_distinct(DMpDistinct A) {
    __shared__ uint4 s_lo[256], s_hi[256];
    const int tid = threadIdx.x, i = tid & (ORBX_MP_GROUP - 1), g0 = tid & ~(ORBX_MP_GROUP - 1);
    const int slot = blockIdx.x * (256 / ORBX_MP_GROUP) + (tid >> 4);
    int p = -1, N = 0;
    long long b = 0;
    if (slot < A.count) {
        p = A.order[slot];
        b = A.obs_begin[p];
        N = min(A.obs_begin[p + 1] - (int)b, (int)ORBX_MP_GROUP);   // the plan sends no larger point here
    }
    uint4 qa = make_uint4(0, 0, 0, 0), qb = qa;
    if (i < N) { const uint4 *r = mp_row(A, b + i); qa = r[0]; qb = r[1]; }
    s_lo[tid] = qa; s_hi[tid] = qb;
    orbx_wave_sync();                                               // a group lies inside one wave
    uint32_t dd[ORBX_MP_GROUP / 2];
#pragma unroll
    for (int w = 0; w < ORBX_MP_GROUP / 2; ++w) {
        const uint32_t d0 = mp_dist(qa, qb, s_lo[g0 + 2 * w], s_hi[g0 + 2 * w]);
        const uint32_t d1 = mp_dist(qa, qb, s_lo[g0 + 2 * w + 1], s_hi[g0 + 2 * w + 1]);
        dd[w] = (2 * w < N ? d0 : 0xffffu) | (2 * w + 1 < N ? d1 : 0xffffu) << 16;
    }
    const uint32_t need = (uint32_t)((N - 1) >> 1) + 1u;
    uint32_t lo = 0, hi = 256;
#pragma unroll 1
    for (int step = 0; step < 9; ++step) {                          // 257 values: nine halvings; lo == hi stays put
        const uint32_t mid = (lo + hi) >> 1;
        uint32_t cnt = 0;
#pragma unroll
        for (int w = 0; w < ORBX_MP_GROUP / 2; ++w) cnt += ((dd[w] & 0xffffu) <= mid ? 1u : 0u) + ((dd[w] >> 16) <= mid ? 1u : 0u);
        const bool ge = cnt >= need;
        hi = ge ? mid : hi;
        lo = ge ? lo : mid + 1;
    }
    uint32_t key = i < N ? lo << 22 | (uint32_t)i : 0xffffffffu;
    key = orbx_row16_min(key);
    if (p >= 0 && N > 0) {
        const int best = (int)(key & 0x3fffffu);
        if (i == 0) { A.best_idx[p] = best; A.best_median[p] = (int)(key >> 22); }
        if (i == 1) A.best_desc[2 * (long long)p] = s_lo[g0 + best];
        if (i == 2) A.best_desc[2 * (long long)p + 1] = s_hi[g0 + best];
    }
}
// Every other N: one workgroup per point, one wave per row i of D (rows i = wave, wave + 4, ...), lane l holding D[i][64 s + l]
// in register s.  The count of a bisection step is a sum of ballots, so the bisection is wave-uniform.  The point's descriptors
// are staged in LDS as two planes of 16 bytes (consecutive lanes read consecutive slots) while N <= ORBX_MP_LDS_ROWS; a larger
// point keeps nothing and recomputes its row from global memory in each step, which is correct for any N.
__global__ __launch_bounds__(256) void k_mp_distinct_wide(DMpDistinct A) {
    __shared__ uint4 s_lo[ORBX_MP_LDS_ROWS], s_hi[ORBX_MP_LDS_ROWS];
    __shared__ unsigned long long s_key[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if ((int)blockIdx.x >= A.count) return;
    const int p = A.order[blockIdx.x];
    const long long b = A.obs_begin[p];
    const int N = A.obs_begin[p + 1] - (int)b;
    if (N <= 0) return;                                             // (uniform; the plan sends no such point)
    const bool staged = N <= ORBX_MP_LDS_ROWS;
    if (staged)
        for (int r = tid; r < N; r += 256) { const uint4 *g = mp_row(A, b + r); s_lo[r] = g[0]; s_hi[r] = g[1]; }
    __syncthreads();
    const uint32_t need = (uint32_t)((N - 1) >> 1) + 1u;
    const int ns = (N + 63) >> 6;
    unsigned long long best = ~0ull;
    for (int i = wave; i < N; i += 4) {
        uint32_t lo = 0, hi = 256;
        if (staged) {
            const uint4 qa = s_lo[i], qb = s_hi[i];
            uint32_t dd[ORBX_MP_SLOTS];
#pragma unroll
            for (int s = 0; s < ORBX_MP_SLOTS; ++s) {
                dd[s] = 0xffffu;
                if (s < ns) {
                    const int j = s * 64 + lane;
                    if (j < N) dd[s] = mp_dist(qa, qb, s_lo[j], s_hi[j]);
                }
            }
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                uint32_t cnt = 0;
#pragma unroll
                for (int s = 0; s < ORBX_MP_SLOTS; ++s)
                    if (s < ns) cnt += (uint32_t)__popcll(orbx_ballot(dd[s] <= mid));
                if (cnt >= need) hi = mid; else lo = mid + 1;
            }
        } else {
            const uint4 *q = mp_row(A, b + i);
            const uint4 qa = q[0], qb = q[1];
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                uint32_t cnt = 0;
                for (int j0 = 0; j0 < N; j0 += 64) {
                    const int j = j0 + lane;
                    bool le = false;
                    if (j < N) { const uint4 *t = mp_row(A, b + j); le = mp_dist(qa, qb, t[0], t[1]) <= mid; }
                    cnt += (uint32_t)__popcll(orbx_ballot(le));
                }
                if (cnt >= need) hi = mid; else lo = mid + 1;
            }
        }
        const unsigned long long key = (unsigned long long)lo << 32 | (uint32_t)i;
        best = key < best ? key : best;                             // rows ascend per wave; the minimum over waves is taken below
    }
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    best = s_key[0];
    for (int w = 1; w < 4; ++w) best = s_key[w] < best ? s_key[w] : best;
    const int bi = (int)(uint32_t)best;
    if (tid == 0) { A.best_idx[p] = bi; A.best_median[p] = (int)(best >> 32); }
    if (tid == 1 || tid == 2) A.best_desc[2 * (long long)p + (tid - 1)] = mp_row(A, b + bi)[tid - 1];
}
// MapPoint::UpdateNormalAndDepth: sixteen lanes per point.  The lanes compute sixteen rows' unit vectors side by side (the
// double square root and divisions are the correctly rounded sequences, as in k_kfdb_score); every lane of the group then adds
// them to its copy of `normal` one after the other in row order: float addition is not associative, so no tree.
__global__ __launch_bounds__(256) void k_mp_normal_depth(const int32_t *__restrict__ obs_begin, const DMpPoint *__restrict__ pts,
                                                         const float *__restrict__ centers, int npoints, float scale_last,
                                                         float *__restrict__ out) {
    const int tid = threadIdx.x, i = tid & 15;
    const int p = blockIdx.x * 16 + (tid >> 4);
    if (p >= npoints) return;                                       // whole groups leave; the shuffles below stay inside a group
    const long long b = obs_begin[p];
    const int N = obs_begin[p + 1] - (int)b;
    if (N <= 0) return;
    const DMpPoint P = pts[p];
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int j0 = 0; j0 < N; j0 += 16) {
        const int j = j0 + i;
        float tx = 0.f, ty = 0.f, tz = 0.f;
        if (j < N) {
            const float *c = centers + 3 * (b + j);
            const float dx = P.pos[0] - c[0], dy = P.pos[1] - c[1], dz = P.pos[2] - c[2];
            double s = 0.0;                                         // cv::norm: a double sum in element order
            s += (double)dx * (double)dx; s += (double)dy * (double)dy; s += (double)dz * (double)dz;
            const double nrm = sqrt(s);
            tx = (float)((double)dx / nrm); ty = (float)((double)dy / nrm); tz = (float)((double)dz / nrm);
        }
        const int cnt = min(16, N - j0);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float vx = __shfl(tx, k, 16), vy = __shfl(ty, k, 16), vz = __shfl(tz, k, 16);
            if (k < cnt) { nx = nx + vx; ny = ny + vy; nz = nz + vz; }
        }
    }
    if (i == 0) {
        const float dx = P.pos[0] - P.ref[0], dy = P.pos[1] - P.ref[1], dz = P.pos[2] - P.ref[2];
        double s = 0.0;
        s += (double)dx * (double)dx; s += (double)dy * (double)dy; s += (double)dz * (double)dz;
        const float dist = (float)sqrt(s);
        const float maxd = dist * P.level_scale;
        float *o = out + 5 * (long long)p;
        o[0] = (float)((double)nx / (double)N); o[1] = (float)((double)ny / (double)N); o[2] = (float)((double)nz / (double)N);
        o[3] = maxd / scale_last;
        o[4] = maxd;
    }
}

#include "orbx_pose.h"
// The ordered term sums of k_pose_opt and k_sim3_opt over one wave's LDS term array (row t at s_term + 65 * t; 65: the summing
// lanes hit different banks) for N unknowns.  Bit k of m stands for COLS consecutive columns from COLS * k on, one edge each.
// add: lane t < TERMS adds its row's columns of the set bits to a, bits and columns ascending -- the reference's edge order, one
// chain per term, no atomics.  share: every lane gets the TERMS sums through s_acc.  The caller's barriers stand between the
// lanes' writes to s_term and add, and after add; m is wave-uniform.  (The one-lane rho0 sums of the chi passes stay in the
// evaluators: routed through here, k_sim3_opt comes out of the compiler with other registers throughout.)
template <int N, int COLS> struct LmSum {
    enum { TERMS = OrbxLm<N>::TERMS };
    static __device__ __forceinline__ double add(const double *s_term, int lane, unsigned long long m, double a) {
        if (lane < TERMS) {
            while (m) {
                const int c = COLS * __builtin_ctzll(m);
                m &= m - 1;
#pragma unroll
                for (int j = 0; j < COLS; ++j) a = orbx_lm_accumulate<N>(lane, a, s_term[lane * 65 + c + j]);
            }
        }
        return a;
    }
    static __device__ __forceinline__ void share(double *s_acc, int lane, double a, double *acc) {
        if (lane < TERMS) s_acc[lane] = a;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TERMS; ++k) acc[k] = s_acc[k];
        __syncthreads();
    }
};
// Optimizer::PoseOptimization, batched (orbx_pose.h): one wave per problem, one problem per workgroup (problems share
// nothing).  The lanes take the frame's features 64 at a time; a lane whose feature carries an active edge computes the edge's
// 28 terms (21 of H, 6 of b, rho0) into LDS, then lane t < 28 adds term t of the chunk's active edges to its accumulator in
// feature order -- the reference's edge order, 28 chains side by side, no atomics.  The 6x6 solve, exp, the pose update and the
// Levenberg-Marquardt bookkeeping (orbx_pose_rounds) run redundantly in every lane on the broadcast sums, so every branch
// around a barrier is uniform.  The outlier flags live in the output row (each lane re-reads what it wrote itself); the stale
// errors of a rejected trial are recomputed from the pose they were taken at.  Every loop is bounded (4 x 10 x 10 passes over
// at most cap features) and nothing waits on another wave.
struct PoseEvDev {
    OrbxPoseView v;
    OrbxPoseCam K;
    uint8_t *outlier;
    double *s_term;     // [28][65]: term t of lane k at t * 65 + k
    double *s_acc;      // [28]
    int lane, nactive;
    __device__ int active() const { return nactive; }
    __device__ void system(const OrbxPoseSE3 &T, bool robust, double *acc) {
        double a = 0.0;
        for (int base = 0; base < v.n; base += 64) {
            const int i = base + lane;
            OrbxPoseEdge e;
            const bool act = i < v.n && orbx_pose_load(v, i, e) && !outlier[i];
            const unsigned long long mask = orbx_ballot(act);
            if (mask == 0ull) continue;
            if (act) {
                double t[ORBX_POSE_TERMS];
                orbx_pose_terms(T, K, e, robust, t);
#pragma unroll
                for (int k = 0; k < ORBX_POSE_TERMS; ++k) s_term[k * 65 + lane] = t[k];
            }
            __syncthreads();
            a = LmSum<6, 1>::add(s_term, lane, mask, a);
            __syncthreads();
        }
        LmSum<6, 1>::share(s_acc, lane, a, acc);
    }
    __device__ double chi(const OrbxPoseSE3 &T, bool robust) {
        double a = 0.0;
        for (int base = 0; base < v.n; base += 64) {
            const int i = base + lane;
            OrbxPoseEdge e;
            const bool act = i < v.n && orbx_pose_load(v, i, e) && !outlier[i];
            const unsigned long long mask = orbx_ballot(act);
            if (mask == 0ull) continue;
            if (act) {
                double pc[3], err[3], rho1;
                s_term[lane] = orbx_pose_huber(orbx_pose_error(T, K, e, pc, err), e.stereo, robust, &rho1);
            }
            __syncthreads();
            if (lane == 0) {
                unsigned long long m = mask;
                while (m) {
                    const int k = __builtin_ctzll(m);
                    m &= m - 1;
                    a = a + s_term[k];
                }
            }
            __syncthreads();
        }
        if (lane == 0) s_acc[0] = a;
        __syncthreads();
        const double r = s_acc[0];
        __syncthreads();
        return r;
    }
    __device__ int classify(const OrbxPoseSE3 &T, const OrbxPoseSE3 &Tlast) {
        int nbad = 0, ngood = 0;
        for (int base = 0; base < v.n; base += 64) {
            const int i = base + lane;
            OrbxPoseEdge e;
            const bool has = i < v.n && orbx_pose_load(v, i, e);
            bool bad = false;
            if (has) {
                double pc[3], err[3];
                const float chi2 = (float)orbx_pose_error(outlier[i] ? T : Tlast, K, e, pc, err);
                bad = chi2 > (e.stereo ? 7.815f : 5.991f);
                outlier[i] = bad ? 1 : 0;
            }
            nbad += __popcll(orbx_ballot(has && bad));
            ngood += __popcll(orbx_ballot(has && !bad));
        }
        nactive = ngood;
        return nbad;
    }
};
__global__ __launch_bounds__(64) void k_pose_opt(const DPoseArgs A) {
    __shared__ double s_term[ORBX_POSE_TERMS * 65];
    __shared__ double s_acc[ORBX_POSE_TERMS];
    const int p = blockIdx.x;
    if (p >= A.nproblems) return;
    const DPoseProb &P = A.prob[p];
    PoseEvDev ev;
    ev.lane = threadIdx.x;
    const int cnt = A.counts[P.frame];
    ev.v.n = cnt < 0 ? 0 : cnt < A.cap ? cnt : A.cap;
    ev.v.kp = A.kps + (long long)P.frame * A.cap;
    ev.v.ur = A.ur ? A.ur + (long long)P.frame * A.cap : nullptr;
    ev.v.pt = A.point + (long long)p * A.cap;
    ev.v.index = P.index_off >= 0 ? A.index + P.index_off : nullptr;
    ev.v.world = A.world;
    ev.v.sig = A.sig;
    ev.v.nlevels = A.nlevels;
    ev.v.npoints = P.npoints;
    ev.K.fx = (double)A.fx; ev.K.fy = (double)A.fy; ev.K.cx = (double)A.cx; ev.K.cy = (double)A.cy; ev.K.bf = (double)A.mbf;
    ev.outlier = A.outlier + (long long)p * A.cap;
    ev.s_term = s_term; ev.s_acc = s_acc;
    int nedges = 0;
    if (A.dbg) {                                               // orbx_debug_pose_inlier_test: the inlier test alone (uniform)
        for (int base = 0; base < ev.v.n; base += 64) {
            const int i = base + ev.lane;
            OrbxPoseEdge e;
            nedges += __popcll(orbx_ballot(i < ev.v.n && orbx_pose_load(ev.v, i, e)));
        }
        float Te[16], Tl[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) { Te[k] = A.dbg[16 * (long long)p + k]; Tl[k] = A.dbg[16 * ((long long)A.nproblems + p) + k]; }
        const int nb = ev.classify(orbx_pose_from_tcw(Te), orbx_pose_from_tcw(Tl));
        if (ev.lane == 0) A.ninliers[p] = nedges - nb;
        return;
    }
    for (int base = 0; base < ev.v.n; base += 64) {           // mvbOutlier[i] = false wherever a MapPoint exists
        const int i = base + ev.lane;
        OrbxPoseEdge e;
        const bool has = i < ev.v.n && orbx_pose_load(ev.v, i, e);
        if (has) ev.outlier[i] = 0;
        nedges += __popcll(orbx_ballot(has));
    }
    ev.nactive = nedges;
    if (nedges < 3) {                                          // (uniform) the pose row stays as it is
        if (ev.lane == 0) A.ninliers[p] = 0;
        return;
    }
    float Tin[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Tin[k] = P.Tcw[k];
    OrbxPoseSE3 T;
    const int nbad = orbx_pose_rounds(ev, Tin, nedges, &T);
    if (ev.lane == 0) {
        float M[16];
        orbx_pose_to_tcw(T, M);
#pragma unroll
        for (int k = 0; k < 16; ++k) A.Tcw[16 * (long long)p + k] = M[k];
        A.ninliers[p] = nedges - nbad;
    }
}

#include "orbx_sim3opt.h"
// Optimizer::OptimizeSim3, batched (orbx_sim3opt.h): one wave per problem, one problem per workgroup, in the anatomy of
// k_pose_opt.  Per linearisation lanes 0..14 build the estimate's and the 14 perturbed Sim3 with their inverses into LDS (the
// same for every edge; every lane then reads them by broadcast).  The lanes take the correspondences 64 at a time; a lane
// whose correspondence is live computes the 36 terms of e12 and of e21, and the chunk goes through the [36][65] term array in
// two halves of 32 correspondences -- column 2 c = e12, column 2 c + 1 = e21 -- so that lane t < 36 adds term t in the
// reference's edge order, e12_i before e21_i, i ascending: 36 chains side by side, no atomics.  The 7x7 solve, exp, the update
// and the Levenberg-Marquardt bookkeeping (orbx_sim3opt_run) run redundantly in every lane on the broadcast sums, so every
// branch around a barrier is uniform.  The live flags are the output keep row (each lane re-reads what it wrote itself).
// Every loop is bounded ((5 + 10) x 10 passes over n correspondences) and nothing waits on another wave.
struct Sim3OptEvDev {
    OrbxSim3OptView v;
    OrbxSim3OptCam K1, K2;
    double th2, delta;
    bool fix_scale;
    uint8_t *keep;
    double *s_term;     // [36][65]: term t of column k at t * 65 + k
    double *s_acc;      // [36]
    double *s_tab;      // [15][16]
    int lane;
    __device__ void system(const OrbxSim3 &S, double *acc) {
        if (lane < ORBX_SIM3OPT_NSIM) orbx_sim3opt_table_entry(S, lane, fix_scale, s_tab + lane * ORBX_SIM3OPT_SIM);
        __syncthreads();
        double a = 0.0;
        for (int base = 0; base < v.n; base += 64) {
            const int i = base + lane;
            const bool act = i < v.n && keep[i];
            const unsigned long long mask = orbx_ballot(act);
            if (mask == 0ull) continue;
            double t12[ORBX_SIM3OPT_TERMS], t21[ORBX_SIM3OPT_TERMS];
            if (act) {
                OrbxSim3OptEdge e12, e21;
                orbx_sim3opt_load(v, i, e12, e21);
                orbx_sim3opt_terms(s_tab, 0, K1, e12, delta, t12);
                orbx_sim3opt_terms(s_tab, 8, K2, e21, delta, t21);
            }
#pragma unroll 1
            for (int half = 0; half < 2; ++half) {
                const unsigned long long hm = (mask >> (32 * half)) & 0xffffffffull;
                if (hm == 0ull) continue;
                if (act && (lane >> 5) == half) {
                    const int c = 2 * (lane & 31);
#pragma unroll
                    for (int k = 0; k < ORBX_SIM3OPT_TERMS; ++k) { s_term[k * 65 + c] = t12[k]; s_term[k * 65 + c + 1] = t21[k]; }
                }
                __syncthreads();
                a = LmSum<7, 2>::add(s_term, lane, hm, a);
                __syncthreads();
            }
        }
        LmSum<7, 2>::share(s_acc, lane, a, acc);
    }
    // the table's entry 0 (S and its inverse), the same in every lane
    __device__ void entry0(const OrbxSim3 &S) {
        if (lane == 0) orbx_sim3opt_table_entry(S, 0, fix_scale, s_tab);
        __syncthreads();
    }
    __device__ double chi(const OrbxSim3 &S) {
        entry0(S);
        double a = 0.0;
        for (int base = 0; base < v.n; base += 64) {
            const int i = base + lane;
            const bool act = i < v.n && keep[i];
            const unsigned long long mask = orbx_ballot(act);
            if (mask == 0ull) continue;
            if (act) {
                OrbxSim3OptEdge e12, e21;
                double err[2], rho1;
                orbx_sim3opt_load(v, i, e12, e21);
                s_term[2 * lane] = orbx_lm_huber(orbx_sim3opt_error(s_tab, K1, e12, err), delta, &rho1);
                s_term[2 * lane + 1] = orbx_lm_huber(orbx_sim3opt_error(s_tab + 8, K2, e21, err), delta, &rho1);
            }
            __syncthreads();
            if (lane == 0) {
                unsigned long long m = mask;
                while (m) {
                    const int k = __builtin_ctzll(m);
                    m &= m - 1;
                    a = a + s_term[2 * k];
                    a = a + s_term[2 * k + 1];
                }
            }
            __syncthreads();
        }
        if (lane == 0) s_acc[0] = a;
        __syncthreads();
        const double r = s_acc[0];
        __syncthreads();
        return r;
    }
    __device__ OrbxSim3 oplus(const OrbxSim3 &S, double *x) const { return orbx_sim3opt_oplus(S, x, fix_scale); }
    __device__ int classify(const OrbxSim3 &Slast) {
        entry0(Slast);
        int nbad = 0;
        for (int base = 0; base < v.n; base += 64) {
            const int i = base + lane;
            const bool act = i < v.n && keep[i];
            bool bad = false;
            if (act) {
                OrbxSim3OptEdge e12, e21;
                double err[2];
                orbx_sim3opt_load(v, i, e12, e21);
                bad = orbx_sim3opt_error(s_tab, K1, e12, err) > th2 || orbx_sim3opt_error(s_tab + 8, K2, e21, err) > th2;
                if (bad) keep[i] = 0;
            }
            nbad += __popcll(orbx_ballot(bad));
        }
        __syncthreads();                                       // the table is free again
        return nbad;
    }
};
__global__ __launch_bounds__(64) void k_sim3_opt(const DSim3OptArgs A) {
    __shared__ double s_mem[ORBX_SIM3OPT_LDS_DOUBLES];
    const int p = blockIdx.x;
    if (p >= A.nproblems) return;
    const DSim3OptProb &P = A.prob[p];
    Sim3OptEvDev ev;
    ev.lane = threadIdx.x;
    ev.s_term = s_mem;
    ev.s_acc = s_mem + ORBX_SIM3OPT_TERMS * 65;
    ev.s_tab = ev.s_acc + ORBX_SIM3OPT_TERMS;
    ev.v.n = P.n < 0 ? 0 : P.n;
    ev.v.pl = A.pts + ORBX_SIM3OPT_PLANES * P.off;
    ev.K1.fx = (double)P.cam1[0]; ev.K1.fy = (double)P.cam1[1]; ev.K1.cx = (double)P.cam1[2]; ev.K1.cy = (double)P.cam1[3];
    ev.K2.fx = (double)P.cam2[0]; ev.K2.fy = (double)P.cam2[1]; ev.K2.cx = (double)P.cam2[2]; ev.K2.cy = (double)P.cam2[3];
    ev.th2 = (double)P.th2;
    ev.delta = (double)(float)sqrt((double)P.th2);
    ev.fix_scale = P.fix_scale != 0;
    ev.keep = A.keep + P.off;
    for (int i = ev.lane; i < ev.v.n; i += 64) ev.keep[i] = 1;
    float R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = P.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = P.t[k];
    const OrbxSim3 init = orbx_sim3opt_from_input(R, t, P.s);
    orbx_sim3opt_result out;
    if (A.inlier_test_only) {                                  // orbx_debug_sim3opt_inlier_test (uniform)
        double l8[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) l8[k] = P.last[k];
        const int nbad = ev.classify(orbx_sim3opt_fetch(l8));
        orbx_sim3opt_store_result(init, ev.v.n - nbad, nbad, ev.v.n, 0, &out);
    } else {
        orbx_sim3opt_run(ev, init, ev.v.n, &out);
    }
    if (ev.lane == 0) A.res[p] = out;
}

#include "orbx_localba.h"
// Optimizer::LocalBundleAdjustment, batched (orbx_localba.h): one workgroup of 256 threads per problem, several problems per
// launch, all arithmetic in double.  The header cuts the work into phases over independent items -- one lane per point walks
// its observations; (keyframe, chain) pairs add the keyframe's edges in 64 interleaved chains; one lane per row of a Schur
// block walks the block's pair list; one lane per row of the reduced system runs its left-looking L D L^T chain, one barrier
// per column -- and the lanes stride over a phase's items with a barrier behind it, so every sum has the order the host path
// gives it.  The Levenberg-Marquardt bookkeeping runs redundantly in every lane on values every lane reads from the same
// places, so every branch around a barrier is uniform.  Everything a phase hands to the next lives in the problem's global
// workspace (L2-resident at the sizes of a local map; the reduced system is not moved into LDS: profiles/localba_batch.md).
// Every loop is bounded ((5 + 10) iterations x 10 trials) and nothing waits on another workgroup.
struct LbaExDev {
    int tid;
    template <class F> __device__ __forceinline__ void each(int n, F f) {
        for (int i = tid; i < n; i += ORBX_LBA_THREADS) f(i);
        __syncthreads();
    }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ bool lead() const { return tid == 0; }
};
__global__ __launch_bounds__(ORBX_LBA_THREADS) void k_local_ba(const DLbaArgs A) {
    const int p = blockIdx.x;
    if (p >= A.nproblems) return;
    const DLbaProb P = A.prob[p];
    OrbxLbaCtx c;
    orbx_localba_bind(P, A.in + P.o_in, A.work + P.o_work, A.out + P.o_out, c);
    LbaExDev ex;
    ex.tid = threadIdx.x;
    orbx_localba_run(ex, c, (orbx_localba_result *)A.out + p);
}

#include "orbx_essgraph.h"
// Optimizer::OptimizeEssentialGraph, batched (orbx_essgraph.h): one workgroup of 256 threads per problem, several problems per
// launch, all arithmetic in double.  The header cuts the work into phases over independent items -- one lane per (edge, side,
// column) takes a central difference and writes one 7-vector of a Jacobian; one lane per (block, row) of the 7 x 7 block-sparse
// system adds its edges; per elimination round one lane per (block, row) forms T, one lane per column factors its 7 x 7
// diagonal block in place, one lane per (block, row) forms L; one lane per column of a round runs the forward and the backward
// solve -- and the lanes stride over a phase's items with a barrier behind it, so every sum has the order the host path gives
// it.  The Levenberg-Marquardt bookkeeping runs redundantly in every lane on values every lane reads from the same places, so
// every branch around a barrier is uniform.  Everything a phase hands to the next lives in the problem's global workspace; no
// lane holds a 7 x 7 block.  Every loop is bounded (20 iterations x 10 trials) and nothing waits on another workgroup.
struct EgExDev {
    int tid;
    template <class F> __device__ __forceinline__ void each(int n, F f) {
        for (int i = tid; i < n; i += ORBX_EG_THREADS) f(i);
        __syncthreads();
    }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ bool lead() const { return tid == 0; }
};
__global__ __launch_bounds__(ORBX_EG_THREADS) void k_essential_graph(const DEgArgs A) {
    const int p = blockIdx.x;
    if (p >= A.nproblems) return;
    const DEgProb P = A.prob[p];
    OrbxEgCtx c;
    orbx_eg_bind(P, A.in + P.o_in, A.work + P.o_work, A.out + P.o_out, c);
    EgExDev ex;
    ex.tid = threadIdx.x;
    orbx_eg_run(ex, c, (orbx_essgraph_result *)A.out + p);
}
// Step 7 of OptimizeEssentialGraph: one lane per map point over all problems of the call, after k_essential_graph on the stream
__global__ __launch_bounds__(256) void k_eg_correct_points(const DEgArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.npoints) return;
    const float *world = (const float *)(A.in + A.o_pts_in);
    const int32_t *ref = (const int32_t *)(world + 3 * A.npoints), *pprob = ref + A.npoints;
    orbx_eg_correct_point(A.prob, A.in, A.out, world, ref, pprob, (float *)(A.out + A.o_pts_out), i);
}

#include "orbx_sim3.h"
// CheckInliers of the batched RANSACs (k_sim3_inliers, k_pnp_inliers): one workgroup = WAVES consecutive hypotheses of ONE
// problem, one wave each.  The problem's points are staged in LDS once per workgroup, CHUNK at a time as PLANES planes (lane i
// reads word i of a plane: no bank conflict); lanes stride over the points, test(v) judges one point from its PLANES staged
// floats, a 64-point word of the mask is one ballot, the count is the sum of the popcounts.  Every barrier is taken by all
// waves (a wave that is not `active`, past the problem's last hypothesis, only stages).
template <int PLANES, int CHUNK, int WAVES, class Test>
__device__ __forceinline__ int ransac_inliers(float *s_pts, const float *pl, int n, bool active, unsigned long long *mw, Test test) {
    const int lane = threadIdx.x & 63;
    int cnt = 0;
    for (int base = 0; base < n; base += CHUNK) {
        const int len = n - base < CHUNK ? n - base : CHUNK;
        __syncthreads();                                       // the previous chunk has been read by every wave
#pragma unroll
        for (int p = 0; p < PLANES; ++p)
            for (int i = threadIdx.x; i < len; i += 64 * WAVES) s_pts[p * CHUNK + i] = pl[(long long)p * n + base + i];
        __syncthreads();
        if (!active) continue;
        for (int sub = 0; sub < len; sub += 64) {
            const int i = sub + lane;                          // < CHUNK; entries at or past len are masked below
            float v[PLANES];
#pragma unroll
            for (int p = 0; p < PLANES; ++p) v[p] = s_pts[p * CHUNK + i];
            const bool in = i < len && test(v);
            const unsigned long long word = orbx_ballot(in);
            if (lane == 0) mw[(base + sub) >> 6] = word;
            cnt += __popcll(word);
        }
    }
    return cnt;
}
// Sim3Solver RANSAC, batched (orbx_sim3.h).  k_sim3_hypotheses: one lane per (problem, iteration) gathers the three drawn
// correspondences and runs ComputeSim3 in registers (the Jacobi sweeps and every 3x3 product are unrolled: no per-thread array
// is indexed at run time), then stores the hypothesis.  The lanes of a wave share no data and take no barrier, so the sweep
// count may differ between them.
__global__ __launch_bounds__(64) void k_sim3_hypotheses(const DSim3Args A) {
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= A.total_hyps) return;
    const DSim3Prob &D = A.prob[A.hyp_prob[h]];
    const float *pl = A.pts + D.pts_off;
    const long long n = D.n;
    float P1[9], P2[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long idx = A.sets[3 * (long long)h + c];    // inside [0, n): checked on the host before the upload
#pragma unroll
        for (int r = 0; r < 3; ++r) { P1[3 * c + r] = pl[r * n + idx]; P2[3 * c + r] = pl[(3 + r) * n + idx]; }
    }
    OrbxSim3Hyp H;
    orbx_sim3_compute(P1, P2, D.fix_scale, H);
    float *o = (float *)(A.hyp + h);
#pragma unroll
    for (int k = 0; k < 16; ++k) { o[k] = H.T12[k]; o[16 + k] = H.T21[k]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) o[32 + k] = H.R[k];
    o[41] = H.t[0]; o[42] = H.t[1]; o[43] = H.t[2]; o[44] = H.s; o[45] = 0.f; o[46] = 0.f; o[47] = 0.f;
}
// k_sim3_inliers: CheckInliers (ransac_inliers) with the wave's T12, T21 and both cameras in registers.
__global__ __launch_bounds__(64 * ORBX_SIM3_WAVES) void k_sim3_inliers(const DSim3Args A) {
    __shared__ float s_pts[ORBX_SIM3_PLANES * ORBX_SIM3_CHUNK];
    const int g = blockIdx.x;
    if (g >= A.ngroups) return;
    const DSim3Prob &D = A.prob[A.groups[2 * g]];
    const int lane = threadIdx.x & 63;
    const int it = A.groups[2 * g + 1] + (threadIdx.x >> 6);
    const bool active = it < D.iterations;                     // (wave-uniform)
    const int n = D.n;
    const float *pl = A.pts + D.pts_off;
    float T12[12], T21[12], K1[4], K2[4];
    {
        const OrbxSim3Hyp &H = A.hyp[D.iter_off + (active ? it : 0)];
#pragma unroll
        for (int k = 0; k < 12; ++k) { T12[k] = H.T12[k]; T21[k] = H.T21[k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { K1[k] = D.K1[k]; K2[k] = D.K2[k]; }
    }
    unsigned long long *mw = A.masks + D.word_off + (long long)(active ? it : 0) * D.nwords;
    const int cnt = ransac_inliers<ORBX_SIM3_PLANES, ORBX_SIM3_CHUNK, ORBX_SIM3_WAVES>(s_pts, pl, n, active, mw, [&](const float *v) {
        return orbx_sim3_inlier(T12, T21, K1, K2, v, v + 3, v + 8, v + 10, v[6], v[7]); });
    if (active && lane == 0) A.tally[D.iter_off + it] = cnt;
}

#include "orbx_pnp.h"
// PnPsolver RANSAC, batched (orbx_pnp.h).  k_pnp_hypotheses: one lane per (problem, iteration) runs compute_pose (EPnP) on the
// four drawn correspondences.  The 12 x 12 MtM and its eigenvectors alone are 288 doubles, more than a lane's registers hold, so
// every array of the algorithm lives in the lane's slice of an LDS workspace: element e of lane l at double index
// e * ORBX_PNP_HYP_LANES + l, which makes every 64-bit LDS access of the wave conflict-free.  ORBX_PNP_HYP_LANES = 32 lanes per
// workgroup keep the workspace (544 doubles per lane, 136 KiB) inside the 160 KiB of a CU.  The lanes share no data and take
// no barrier, so sweep counts may differ between them.  The job is a few hundred to a few thousand hypotheses: latency-bound.
__global__ __launch_bounds__(ORBX_PNP_HYP_LANES) void k_pnp_hypotheses(const DPnpArgs A) {
    __shared__ double s_ws[ORBX_PNP_WS_DOUBLES(4) * ORBX_PNP_HYP_LANES];
    const int h = blockIdx.x * ORBX_PNP_HYP_LANES + threadIdx.x;
    if (h >= A.total_hyps) return;
    const DPnpProb &D = A.prob[A.hyp_prob[h]];
    const float *pl = A.pts + D.pts_off;
    const long long n = D.n;
    const OrbxPnpWs W = {s_ws + threadIdx.x, ORBX_PNP_HYP_LANES};
    for (int c = 0; c < 4; ++c) {
        const long long idx = A.sets[4 * (long long)h + c];    // inside [0, n): checked on the host before the upload
        for (int r = 0; r < 3; ++r) W(ORBX_PNP_FIXED + 3 * c + r) = (double)pl[r * n + idx];
        W(ORBX_PNP_FIXED + 12 + 2 * c) = (double)pl[3 * n + idx];
        W(ORBX_PNP_FIXED + 12 + 2 * c + 1) = (double)pl[4 * n + idx];
    }
    const double cam[4] = {D.cam[0], D.cam[1], D.cam[2], D.cam[3]};
    OrbxPnpHyp &H = A.hyp[h];
    const int N = orbx_pnp_compute_pose(W, 4, cam, H.R);       // R (9) | t (3) are contiguous in the record
    orbx_pnp_store(H.R, N, H);
}
// k_pnp_inliers: CheckInliers (ransac_inliers) with the wave's R, t and the camera in registers, as doubles.
__global__ __launch_bounds__(64 * ORBX_PNP_WAVES) void k_pnp_inliers(const DPnpArgs A) {
    __shared__ float s_pts[ORBX_PNP_PLANES * ORBX_PNP_CHUNK];
    const int g = blockIdx.x;
    if (g >= A.ngroups) return;
    const DPnpProb &D = A.prob[A.groups[2 * g]];
    const int lane = threadIdx.x & 63;
    const int it = A.groups[2 * g + 1] + (threadIdx.x >> 6);
    const bool active = it < D.iterations;                     // (wave-uniform)
    const int n = D.n;
    const float *pl = A.pts + D.pts_off;
    double R[9], t[3], cam[4];
    {
        const OrbxPnpHyp &H = A.hyp[D.iter_off + (active ? it : 0)];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = H.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = H.t[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) cam[k] = D.cam[k];
    }
    unsigned long long *mw = A.masks + D.word_off + (long long)(active ? it : 0) * D.nwords;
    const int cnt = ransac_inliers<ORBX_PNP_PLANES, ORBX_PNP_CHUNK, ORBX_PNP_WAVES>(s_pts, pl, n, active, mw, [&](const float *v) {
        return orbx_pnp_inlier(R, t, cam, v[0], v[1], v[2], v[3], v[4], v[5]); });
    if (active && lane == 0) A.tally[D.iter_off + it] = cnt;
}

#include "orbx_init.h"
// Initializer H / F RANSAC, batched (orbx_init.h).  k_init_hypotheses: one lane per (problem, model, iteration) runs the
// eight-point DLT of ComputeH21 / ComputeF21 and what FindHomography / FindFundamental do with its result.  A (16 x 9) and V
// (9 x 9) are indexed by the Jacobi's run-time column pair, so they live in the lane's slice of an LDS workspace: element e of
// lane l at float index e * ORBX_INIT_HYP_LANES + l, which makes every 32-bit LDS access of the wave conflict-free.
// ORBX_INIT_HYP_LANES = 64 lanes (one wave) take 257 floats each, 64.25 KiB per workgroup, so two workgroups share a CU's
// 160 KiB; more lanes per workgroup would not put more waves on a CU, the LDS per lane is the limit.  The lanes share no
// data and take no barrier, so sweep counts may differ between them.
__global__ __launch_bounds__(ORBX_INIT_HYP_LANES) void k_init_hypotheses(const DInitArgs A) {
    __shared__ float s_ws[ORBX_INIT_WS_FLOATS * ORBX_INIT_HYP_LANES];
    const int h = blockIdx.x * ORBX_INIT_HYP_LANES + threadIdx.x;
    if (h >= A.total_hyps) return;
    const DInitProb &D = A.prob[A.hyp_prob[h]];
    const int l = h - D.hyp_off;
    const bool is_h = orbx_init_is_h(D, l);
    const float *pl = A.pts + D.pts_off;
    const long long n = D.n;
    const int32_t *set = A.sets + D.set_off + 8 * (long long)orbx_init_iteration(D, l);
    const OrbxInitWs W = {s_ws + threadIdx.x, ORBX_INIT_HYP_LANES};
    for (int c = 0; c < 8; ++c) {
        const long long idx = set[c];                          // inside [0, n): checked on the host before the upload
        for (int r = 0; r < 4; ++r) W(ORBX_INIT_PTS + 4 * c + r) = pl[r * n + idx];
    }
    orbx_init_hypothesis(W, is_h, D.T1, is_h ? D.T2inv : D.T2t, A.hyp[h]);
}
// k_init_scores: CheckHomography / CheckFundamental.  One workgroup = one wave = ORBX_INIT_SCORE_LANES consecutive hypotheses of
// ONE problem, one LANE each: the lane keeps its matrix in registers and walks the matches in order, so the score is the
// source's sequential float sum by construction and every lane works through the whole fold.  The un-normalised matches are
// staged in LDS ORBX_INIT_CHUNK at a time and read back as broadcasts (every lane reads the same address).  A lane collects 64
// inlier bits in a register and stores the word when it is full and after the last match.  Not ransac_inliers: one lane (not
// one wave) per hypothesis, a sequential sum, broadcast reads.
__global__ __launch_bounds__(ORBX_INIT_SCORE_LANES) void k_init_scores(const DInitArgs A) {
    __shared__ float s_pts[4 * ORBX_INIT_CHUNK];
    const int g = blockIdx.x;
    if (g >= A.ngroups) return;
    const DInitProb &D = A.prob[A.groups[2 * g]];
    const int nh = orbx_init_nhyp(D);
    const int l0 = A.groups[2 * g + 1] + threadIdx.x;
    const bool active = l0 < nh;
    const int l = active ? l0 : nh - 1;                         // a lane past the problem's last hypothesis repeats it and stores nothing
    const bool is_h = orbx_init_is_h(D, l);
    const int n = D.n;
    const float *pl = A.pts + D.pts_off + 4 * (long long)n;     // planes 4 .. 7: the raw u1 v1 u2 v2
    float M[9], Mi[9];
    {
        const OrbxInitHyp &H = A.hyp[D.hyp_off + l];
#pragma unroll
        for (int k = 0; k < 9; ++k) { M[k] = H.M[k]; Mi[k] = H.Minv[k]; }
    }
    const float inv_sigma2 = D.inv_sigma2;
    unsigned long long *mw = A.masks + D.word_off + (long long)l * D.nwords;
    float score = 0.0f;
    unsigned long long word = 0;
    for (int base = 0; base < n; base += ORBX_INIT_CHUNK) {
        const int len = n - base < ORBX_INIT_CHUNK ? n - base : ORBX_INIT_CHUNK;
        __syncthreads();                                       // the previous chunk has been read by every lane
#pragma unroll
        for (int p = 0; p < 4; ++p)
            for (int i = threadIdx.x; i < len; i += ORBX_INIT_SCORE_LANES) s_pts[p * ORBX_INIT_CHUNK + i] = pl[(long long)p * n + base + i];
        __syncthreads();
        for (int i = 0; i < len; ++i) {
            const float u1 = s_pts[i], v1 = s_pts[ORBX_INIT_CHUNK + i], u2 = s_pts[2 * ORBX_INIT_CHUNK + i], v2 = s_pts[3 * ORBX_INIT_CHUNK + i];
            const bool in = is_h ? orbx_init_check_h(M, Mi, u1, v1, u2, v2, inv_sigma2, score)
                                 : orbx_init_check_f(M, u1, v1, u2, v2, inv_sigma2, score);
            const int m = base + i;
            if (in) word |= 1ull << (m & 63);
            if ((m & 63) == 63 || m + 1 == n) {
                if (active) mw[m >> 6] = word;
                word = 0;
            }
        }
    }
    if (active) A.tally[D.hyp_off + l] = orbx_canonf(score);
}

#include "orbx_recon.h"
// ReconstructH / ReconstructF, batched (orbx_recon.h).  k_init_decompose: one lane per problem forms E21 or A, takes the 3 x 3
// SVD -- its columns are picked at run time, so the matrix and its V live in the lane's slice of an LDS workspace, element e of
// lane l at float index e * ORBX_RECON_LANES + l -- and stores the problem's 4 or 8 pose records.  The lanes share no data and
// take no barrier.
__global__ __launch_bounds__(ORBX_RECON_LANES) void k_init_decompose(const DReconArgs A) {
    __shared__ float s_ws[ORBX_RECON_WS_FLOATS * ORBX_RECON_LANES];
    const int j = blockIdx.x * ORBX_RECON_LANES + threadIdx.x;
    if (j >= A.nlaunch) return;
    const DReconProb &D = A.prob[j];
    const OrbxInitWs W = {s_ws + threadIdx.x, ORBX_RECON_LANES};
    float M[9], K[4];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = D.M[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) K[k] = D.K[k];
    OrbxReconPose *out = A.pose + (long long)ORBX_RECON_MAX_HYP * j;
    if (D.nhyp == 0) return;                                    // fused call: ORBX_INIT_NONE, nothing of this problem is read
    if (D.is_h) orbx_recon_decompose_h(W, M, K, out);
    else orbx_recon_decompose_f(W, M, K, out);
}
// k_init_check_rt: CheckRT with Triangulate.  One workgroup = one wave = one (problem, pose hypothesis); lane l takes the matches
// l, l + 64, ...  Per match it writes the status byte, the point and the cosine into the hypothesis' planes (zeros where nothing
// is stored); nGood is the sum of the ballot population counts, the same whatever the lane order.  The order statistic
// vCosParallax[min(50, nGood - 1)] is selected by value: the largest key K with #{key < K} <= idx, built bit by bit from the top
// in 32 steps, each a ballot count over the cosines -- every lane reads back only what it wrote itself.  No LDS, no atomics.
__global__ __launch_bounds__(64) void k_init_check_rt(const DReconArgs A) {
    const int h = blockIdx.x, j = h / ORBX_RECON_MAX_HYP, i = h % ORBX_RECON_MAX_HYP;
    if (j >= A.nlaunch) return;
    const DReconProb &D = A.prob[j];
    if (i >= D.nhyp) return;                                    // slots 4 .. 7 of an F problem; every slot of a problem without a model
    const int n = D.n, lane = threadIdx.x;
    const OrbxReconPose P = A.pose[h];
    float K[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) K[k] = D.K[k];
    const float th2 = D.th2;
    const long long plane = (long long)ORBX_RECON_MAX_HYP * D.m_off + (long long)i * n;
    uint8_t *st = A.all_st + plane;
    float *pts = A.all_pts + 3 * plane, *cs = A.all_cos + plane;
    const float *pl = A.keys + D.key_off;
    const uint8_t *inl = A.inl + D.m_off;
    int nGood = 0;
    for (int base = 0; base < n; base += 64) {
        const int m = base + lane;
        int s = 0;
        float pt[3] = {0.0f, 0.0f, 0.0f}, c = 0.0f;
        if (m < n && P.valid && inl[m])
            s = orbx_recon_check_match(P, K, th2, pl[m], pl[(long long)n + m], pl[2 * (long long)n + m], pl[3 * (long long)n + m], pt, c);
        const bool counted = s >= 2;
        if (m < n) {
            st[m] = (uint8_t)s;
            pts[3 * (long long)m] = counted ? pt[0] : 0.0f;
            pts[3 * (long long)m + 1] = counted ? pt[1] : 0.0f;
            pts[3 * (long long)m + 2] = counted ? pt[2] : 0.0f;
            cs[m] = counted ? c : 0.0f;
        }
        nGood += __popcll(__ballot(counted));
    }
    float cosine = 0.0f;
    if (nGood > 0) {                                            // wave-uniform
        const int idx = nGood - 1 < ORBX_RECON_IDX ? nGood - 1 : ORBX_RECON_IDX;
        uint32_t key = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t trial = key | (1u << bit);
            int below = 0;
            for (int base = 0; base < n; base += 64) {
                const int m = base + lane;
                const bool lt = m < n && st[m] >= 2 && orbx_recon_key(cs[m]) < trial;
                below += __popcll(__ballot(lt));
            }
            if (below <= idx) key = trial;
        }
        cosine = orbx_recon_unkey(key);
    }
    if (lane == 0) {
        OrbxReconTally T;
        T.nGood = nGood; T.cosine = cosine;
        A.tally[h] = T;
    }
}
// k_init_select (the fused call only): one wave per problem that launched its RANSAC.  Per requested model the first strict
// maximum of the scores from 0 -- each lane keeps the first strict maximum of the iterations l, l + 64, ... it visits in
// ascending order, the wave takes the largest of those and, among equal ones, the lowest iteration; a NaN never wins --, then RH
// and the model (orbx_recon_choose), and the reconstruction's record: is_h, nhyp, the winning matrix, and the winning mask
// unpacked into the problem's inlier bytes.  Without a model nhyp stays 0 and the inlier bytes are cleared.
__global__ __launch_bounds__(64) void k_init_select(const DInitArgs I, const DReconArgs A) {
    const int j = blockIdx.x;
    if (j >= A.nlaunch) return;
    const DInitProb &D = I.prob[j];
    const int lane = threadIdx.x, n = D.n;
    float S[2] = {0.0f, 0.0f};
    int it[2] = {-1, -1};
#pragma unroll
    for (int mo = 0; mo < 2; ++mo) {
        if (!(D.models & (1 << mo))) continue;
        const float *sc = I.tally + D.hyp_off + ((mo == 1 && (D.models & 1)) ? D.iterations : 0);
        float best = 0.0f;
        int at = -1;
        for (int l = lane; l < D.iterations; l += 64) {
            const float s = sc[l];
            if (s > best) { best = s; at = l; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ob = __shfl_xor(best, d);
            const int oa = __shfl_xor(at, d);
            if (oa >= 0 && (at < 0 || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
        }
        S[mo] = best; it[mo] = at;
    }
    const int model = orbx_recon_choose(S[0], S[1], it[0], it[1]);
    DReconProb &R = A.prob[j];
    uint8_t *inl = A.inl + R.m_off;
    if (model == ORBX_INIT_NONE) {
        for (int m = lane; m < n; m += 64) inl[m] = 0;
        return;
    }
    const bool is_h = model == ORBX_INIT_H;
    const int l = (is_h || !(D.models & 1) ? 0 : D.iterations) + (is_h ? it[0] : it[1]);
    const unsigned long long *mw = I.masks + D.word_off + (long long)l * D.nwords;
    for (int m = lane; m < n; m += 64) inl[m] = (uint8_t)((mw[m >> 6] >> (m & 63)) & 1ull);
    if (lane < 9) R.M[lane] = I.hyp[D.hyp_off + l].M[lane];
    if (lane == 0) { R.is_h = is_h ? 1 : 0; R.nhyp = is_h ? 8 : 4; }
}
// k_init_pick: one wave per problem.  Which hypothesis can win depends on the counts alone (orbx_recon_candidate); only its status
// and point planes go into the block that is downloaded, zeros when there is none.
__global__ __launch_bounds__(64) void k_init_pick(const DReconArgs A) {
    const int j = blockIdx.x;
    if (j >= A.nlaunch) return;
    const DReconProb &D = A.prob[j];
    const int n = D.n, lane = threadIdx.x;
    const int c = D.nhyp == 0 ? -1 : orbx_recon_candidate(D.is_h != 0, A.tally + (long long)ORBX_RECON_MAX_HYP * j);
    if (lane == 0) A.chosen[j] = c;
    const long long plane = (long long)ORBX_RECON_MAX_HYP * D.m_off + (long long)(c >= 0 ? c : 0) * n;
    const uint8_t *st = A.all_st + plane;
    const float *pts = A.all_pts + 3 * plane;
    uint8_t *ost = A.st + D.m_off;
    float *opts = A.pts + 3 * (long long)D.m_off;
    for (int m = lane; m < n; m += 64) ost[m] = c >= 0 ? st[m] : (uint8_t)0;
    for (int e = lane; e < 3 * n; e += 64) opts[e] = c >= 0 ? pts[e] : 0.0f;
}

// ---------------------------------------------------------------- LocalMapping::CreateNewMapPoints, the per-match geometry
#include "orbx_newpoints.h"
// k_new_points: one workgroup = one wave = one chunk of ORBX_NEWPTS_CHUNK matches of ONE problem (the chunk table of the upload),
// one lane per match.  The chunk and with it the problem record come from blockIdx alone, so the two cameras are wave-uniform and
// arrive through scalar loads; the per-match operands are the host's gathered planes, read coalesced.  orbx_newpoints_match keeps
// the 4 x 4 system and its V in registers.  A lane past the problem's last match does nothing: no barrier, no cross-lane
// operation follows.  Every match of the call is written exactly once: the status byte and the point (zeros when rejected).
__global__ __launch_bounds__(ORBX_NEWPTS_CHUNK) void k_new_points(const DNewPtsArgs A) {
    const int c = blockIdx.x;
    if (c >= A.nchunks) return;
    const DNewPtsChunk ch = A.chunk[c];
    const DNewPtsProb &D = A.prob[ch.prob];
    const int m = ch.base + (int)threadIdx.x;
    if (m >= D.n) return;
    const long long g = (long long)D.m_off + m, total = A.total;
    float pt[3];
    const int s = orbx_newpoints_match(D.c1, D.c2, D.ratio_factor, orbx_newpoints_obs(A.planes, total, g, 0),
                                       orbx_newpoints_obs(A.planes, total, g, 1), pt);
    A.st[g] = (uint8_t)s;
    A.pts[3 * g] = pt[0];
    A.pts[3 * g + 1] = pt[1];
    A.pts[3 * g + 2] = pt[2];
}

// ---------------------------------------------------------------- ORBmatcher::SearchBySim3, batched, pose algebra included
#include "orbx_sim3search.h"
// k_sim3s_project: one thread per (problem, direction, feature) -- blockIdx.y = 2 * problem + direction, so the problem record
// and the direction's pose arrive through scalar loads.  orbx_sim3s_project (the shared header) gives the status, the
// projection, the level and the window; a point that reaches the search becomes a DTrackQ and its query index is appended to the
// compacted list of live queries (ballot, one atomic per wave: the list's order is arbitrary, every query's result is its own).
// Most features of a keyframe are not searched -- no point, or already matched -- and never cost a wave in k_sim3s_cand.
__global__ __launch_bounds__(256) void k_sim3s_project(const DSim3sArgs A) {
    const int k = blockIdx.y >> 1, d = blockIdx.y & 1;
    const DSim3sProb &D = A.prob[k];
    if (d == 0 && blockIdx.x == 0 && threadIdx.x == 0) A.nfound[k] = 0;   // k_sim3s_mutual adds to it, launches later
    const int n = D.n[d];
    if ((int)(blockIdx.x * 256) >= n) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int g = D.q_off + (d ? D.n[0] : 0) + i;
    bool live = false;
    if (i < n) {
        const DSim3sPt T = A.pt[(long long)D.kf[d] * A.fstride + i];
        OrbxSim3sProj o;
        o.status = ORBX_SIM3S_NOT_SEARCHED; o.u = 0.0f; o.v = 0.0f; o.r = -1.0f; o.level = -1;
        if (T.has && !A.flag[g]) o = orbx_sim3s_project(D.dir[d], A.cam, D.th, T);
        live = o.status == ORBX_SIM3S_NO_CANDIDATE;
        A.status[g] = (uint8_t)o.status;
        A.level[g] = o.level;
        A.best[g] = -1;
        *(float2 *)(A.uv + 2 * (long long)g) = make_float2(o.u, o.v);
        if (live) {
            DTrackQ Q;
            Q.x = o.u; Q.y = o.v; Q.ur = 0.0f; Q.r = o.r;
            Q.min_level = o.level - 1; Q.max_level = o.level;      // max_level >= 0: track_scan applies the band [level - 1, level]
            Q.obs = 0; Q.angle = 0.0f; Q.prob = k; Q.pad = d;
            A.q[g] = Q;
        }
    }
    const unsigned long long m = orbx_ballot(live);
    int base = 0;
    if ((threadIdx.x & 63) == 0 && m) base = atomicAdd(A.ctr, (int)__popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    if (live) A.live[base + orbx_wave_rank(m)] = g;
}
// k_sim3s_cand: a bounded grid of waves strides over the live queries; each runs track_scan<false> (GetFeaturesInArea's bucket
// walk with the level band, the smallest key dist << 16 | visiting position = the first strict minimum) against the target
// keyframe's grid, with the MapPoint's descriptor read where the pool holds it, and writes vnMatch and the final status.
__global__ __launch_bounds__(256) void k_sim3s_cand(const DSim3sArgs A, const DGrid gp) {
    const int lane = threadIdx.x & 63;
    const int nlive = min(A.ctr[0], A.nq), nw = gridDim.x * 4;
    for (int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); w < nlive; w += nw) {
        const int g = __builtin_amdgcn_readfirstlane(A.live[w]);
        const DTrackQ Q = A.q[g];
        const int k = __builtin_amdgcn_readfirstlane(Q.prob), d = __builtin_amdgcn_readfirstlane(Q.pad) & 1;
        const DSim3sProb &D = A.prob[k];
        const long long src = D.kf[d], tgt = D.kf[1 - d];
        const int i = g - D.q_off - (d ? D.n[0] : 0);
        const uint4 *qp = (const uint4 *)(A.pdesc + (src * A.fstride + i) * 32);
        const TrackBest B = track_scan<false>(gp, Q, qp[0], qp[1], A.keys + tgt * A.fstride, A.desc + tgt * A.fstride * 32, nullptr,
                                              A.cb + tgt * (GR_CELLS + 1), A.items + tgt * A.fstride, min(A.cnt[tgt], A.fstride),
                                              nullptr, lane);
        if (lane == 0) {
            int32_t best;
            A.status[g] = (uint8_t)orbx_sim3s_outcome(B.k1, (int)(B.p1 & 0xffffu), &best);
            A.best[g] = best;
        }
    }
}
// k_sim3s_mutual: one thread per KF1 feature (blockIdx.y = problem): the agreement test of :1667-1681, the count by ballot and
// one atomic per wave.
__global__ __launch_bounds__(256) void k_sim3s_mutual(const DSim3sArgs A) {
    const int k = blockIdx.y;
    const DSim3sProb &D = A.prob[k];
    const int n1 = D.n[0];
    if ((int)(blockIdx.x * 256) >= n1) return;
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    bool both = false;
    if (i1 < n1) {
        const int idx2 = A.best[D.q_off + i1];
        both = idx2 >= 0 && idx2 < D.n[1] && A.best[D.q_off + n1 + idx2] == i1;
        A.matches[D.m_off + i1] = both ? idx2 : -1;
    }
    const unsigned long long m = orbx_ballot(both);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(A.nfound + k, (int)__popcll(m));
}

// ------------------------------------------------------------------------------------------------
// launch wrappers (called from the C ABI units)
// ------------------------------------------------------------------------------------------------
#include "orbx_launch.h"
#include <string>
#include <cstdio>
#include <cstring>
#include <mutex>

void orbx_pattern_lane_tables(signed char *i8, float *f32) {
    for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r)
            for (int k = 0; k < 4; ++k) i8[l * 16 + r * 4 + k] = ORBX_PATTERN_I8[(r * 64 + l) * 4 + k];
    for (int i = 0; i < 64 * 16; ++i) f32[i] = (float)i8[i];   // |coordinate| <= 127: exact
}
hipError_t orbx_upload_pattern() {
    signed char t[64 * 16];
    static float tf[64 * 16];   // (orbx_pattern_lane_tables fills both forms; the device reads the int8 one alone)
    orbx_pattern_lane_tables(t, tf);
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_pattern_lane), t, sizeof(t));
    if (e != hipSuccess) return e;
    // IC_Angle weight table: umax of the reference's constructor (src/ORBextractor.cc:866-910) for HALF_PATCH_SIZE = 15
    orbx_params p;
    orbx_default_params(&p);
    OrbxTables tab;
    orbx_build_tables(p, tab);
    static uint32_t w[64][12];
    memset(w, 0, sizeof(w));
    for (int lane = 0; lane < 62; ++lane) {
        const int row = lane >> 1, half = lane & 1, v = row - ORBX_HALF_PATCH;
        const int d = tab.umax[v < 0 ? -v : v];
        for (int k = 0; k < 5; ++k)
            for (int b = 0; b < 4; ++b) {
                const int col = 4 * (1 + 5 * half + k) + b;      // byte column inside the 44-byte LDS patch row
                const int u = col - DS_R;
                if (col < DS_W && u >= -d && u <= d) {
                    w[lane][k] |= (uint32_t)(u + 16) << (8 * b);
                    w[lane][5 + k] |= 1u << (8 * b);
                }
            }
    }
    e = hipMemcpyToSymbol(HIP_SYMBOL(c_orient_w), w, sizeof(w));
    if (e != hipSuccess) return e;
    static uint32_t bb[3][64][4];
    memset(bb, 0, sizeof(bb));
    const int K7[7] = {18, 34, 49, 55, 49, 34, 18};   // the 8-bit Gaussian of k_blur / k_describe
    for (int j = 0; j < 3; ++j)
        for (int lane = 0; lane < 64; ++lane)
            for (int sl = 0; sl < 16; ++sl) {
                const int k = 16 * (lane >> 4) + sl, i = k - (16 * j + (lane & 15));
                if (i >= 0 && i <= 6) bb[j][lane][sl >> 2] |= (uint32_t)K7[i] << (8 * (sl & 3));
            }
    return hipMemcpyToSymbol(HIP_SYMBOL(c_blur_b), bb, sizeof(bb));
}

size_t orbx_quadtree_smem(int ncap, int lds_keys) {
    return QT_SHARED_BYTES + (size_t)ncap * (8 * 4 + 16 + 8 + 6 * 4) + 16 + (size_t)lds_keys * 6 + 16;
}

void orbx_launch_clear(hipStream_t s, int *a, int na, int *b, int nb, int *c, int nc) {
    const int n = na > nb ? (na > nc ? na : nc) : (nb > nc ? nb : nc);
    hipLaunchKernelGGL(k_clear, dim3((n + 255) / 256), dim3(256), 0, s, a, na, b, nb, c, nc);
}
void orbx_launch_pyr_l0(hipStream_t s, const DGeom &g, int B, const uint8_t *imgs, int W, int H, int stride,
                        long long frame_stride, uint8_t *pyr, int *status, int *cand_cursor) {
    const DLevel &L = g.lv[0];
    // interior columns [32, xe): the 20-byte aligned window of every 16-pixel chunk stays inside the source row
    int xe = 32;
    while (xe + 1 <= W) xe += 16;           // chunk at X reads source bytes [X - 22, X + 1): must end inside the row
    const int icols = (xe - 32 + 1023) / 1024;
    dim3 grid(B, icols + 1, (L.ph + 4 * L0_ROWS - 1) / (4 * L0_ROWS));
    hipLaunchKernelGGL(k_pyr_l0, grid, dim3(64, 4), 0, s, g, imgs, W, H, stride, frame_stride, pyr, xe, status, cand_cursor);
}
void orbx_launch_pyr_l0_color(hipStream_t s, const DGeom &g, int B, const uint8_t *imgs, int W, int H, int stride,
                              long long frame_stride, uint8_t *pyr, int nch, int r_off, int b_off, int *status, int *cand_cursor) {
    const DLevel &L = g.lv[0];
    dim3 grid((L.pw + 255) / 256, (L.ph + 3) / 4, B);
    hipLaunchKernelGGL(k_pyr_l0_color, grid, dim3(64, 4), 0, s, g, imgs, W, H, stride, frame_stride, pyr, nch, r_off, b_off, status, cand_cursor);
}
void orbx_launch_pyr_l0_remap(hipStream_t s, const DGeom &g, int B, const uint8_t *imgs, int W, int H, int stride,
                              long long frame_stride, uint8_t *pyr, const uint2 *rect, int *status, int *cand_cursor) {
    const DLevel &L = g.lv[0];
    dim3 grid((L.pw + 255) / 256, (L.ph + 3) / 4, B);
    hipLaunchKernelGGL(k_pyr_l0_remap, grid, dim3(64, 4), 0, s, g, imgs, W, H, stride, frame_stride, pyr, rect, status, cand_cursor);
}
// destination rows per wave of the row-walking kernels: 16 when the launch still has >= 4096 waves, fewer for small batches (the
// rows of a wave are a serial chain of load -> evaluate -> store steps); forced (ORBX_RR_RPW: a power of two, 2..64) overrides it.
// Always even: the walk fetches the vertical tap records of rows Y, Y + 1 together.
static int rr_rows_per_wave(const DLevel &L, int B, int forced) {
    if (forced > 0) return forced;
    int rpw = 16;   // (8 / 16 / 32 / 64 rows per wave at 1024 frames: 750 / 708 / 729 / 742 us for the seven launches)
    while (rpw > 2 && (long long)((L.pw + 255) / 256) * ((L.ph + rpw - 1) / rpw) * B < 4096) rpw >>= 1;
    return rpw;
}
void orbx_launch_pyr_resize(hipStream_t s, const DGeom &g, int B, int level, const OrbxTap *taps, uint8_t *pyr, bool narrow,
                            int rpw_forced) {
    const DLevel &L = g.lv[level];
    if (narrow) {
        const int rpw = rr_rows_per_wave(L, B, rpw_forced);
        dim3 grid(B, (L.pw + 255) / 256, (L.ph + RR_WPB * rpw - 1) / (RR_WPB * rpw));
        hipLaunchKernelGGL(k_pyr_resize_rows, grid, dim3(64, RR_WPB), 0, s, g, level, taps, pyr, rpw);
        return;
    }
    dim3 grid((L.pw + 255) / 256, (L.ph + 4 * RS_ROWS - 1) / (4 * RS_ROWS), B);
    hipLaunchKernelGGL(k_pyr_resize, grid, dim3(64, 4), 0, s, g, level, taps, pyr);
}
void orbx_launch_pyr_resize_l1(hipStream_t s, const DGeom &g, int B, const OrbxTap *taps_l1, const OrbxRaw0 &raw, uint8_t *pyr,
                               int tail_bx, int *status, int *cand_cursor, int rpw_forced) {
    const DLevel &L = g.lv[1];
    const int rpw = rr_rows_per_wave(L, B, rpw_forced);
    dim3 grid(B, (L.pw + 255) / 256, (L.ph + RR_WPB * rpw - 1) / (RR_WPB * rpw));
    hipLaunchKernelGGL(k_pyr_resize_rows_l1, grid, dim3(64, RR_WPB), 0, s, g, taps_l1, raw, pyr, rpw, tail_bx, status, cand_cursor);
}
void orbx_launch_fast_rows(hipStream_t s, const DGeom &g, int B, const OrbxCell *cells, const OrbxFastGroup *groups,
                           int ngroups, const uint8_t *pyr, uint2 *cand, int *cand_cursor, int *status, int max_ch, int lcap,
                           int dbg_stop, int lds_floor, const OrbxRaw0 *raw, bool l0_only, int gpw_forced) {
    if (ngroups <= 0) return;
    lcap = (max(lcap, 64) + 1) & ~1;
    // LDS per wave decides how many waves a CU holds: the corner list of a group is sized for its usual load, FR_CCAP entries (the
    // average group has ~130 corners), not for the work list's worst case -- a group with more corners than that runs its NMS as the
    // dense rescan of the score map -- and tile / score map are rounded to 16 bytes, not to four rows.  Bytes per wave (fr_lds) =
    // 2 * map + 2 * lcap + 2 * FR_STACK + 2 * ccap = 2 * map + 2 560 with the default 640-entry work list and 512 corners: 8 192 for
    // 37-row cells (the level-0 launch at 640x480: 20 waves in a CU's 160 KiB), 8 640 / 9 120 for the 40 / 43-row tiles of the
    // launches that carry every level (18 / 17 waves).  512 was chosen by measurement, not by an occupancy step (round 3, second
    // half: 1.316 / 1.319 -> 1.286 / 1.272 ms against 256 entries, because fewer groups take the rescan; 640 entries: 1.39-1.41 ms).
    const int ccap = min(lcap, FR_CCAP);
    const FrLds lds = fr_lds(max_ch, lcap, ccap);
    // lds_floor (the sub-batch pipeline): the request is raised to cap the waves a CU holds, leaving registers for the pyramid
    // kernels of the other stream; the kernel uses no more than it did
    const size_t need = (size_t)lds.bytes;
    const size_t smem = lds_floor > 0 && (size_t)lds_floor > need ? (size_t)lds_floor : need;
    const int gpw = orbx_fast_gpw(B, ngroups, gpw_forced);   // groups per wave (orbx_launch.h)
    if (raw && l0_only)
        hipLaunchKernelGGL(k_fast_rows_l0, dim3(B, (ngroups + gpw - 1) / gpw), dim3(64), smem, s, g, cells, groups, cand,
                           cand_cursor, status, max_ch, lcap, ngroups, gpw, dbg_stop, ccap, *raw);
    else if (raw)
        hipLaunchKernelGGL(k_fast_rows_ip, dim3(B, (ngroups + gpw - 1) / gpw), dim3(64), smem, s, g, cells, groups, pyr, cand,
                           cand_cursor, status, max_ch, lcap, ngroups, gpw, dbg_stop, ccap, *raw);
    else
        hipLaunchKernelGGL(k_fast_rows, dim3(B, (ngroups + gpw - 1) / gpw), dim3(64), smem, s, g, cells, groups, pyr, cand,
                           cand_cursor, status, max_ch, lcap, ngroups, gpw, dbg_stop, ccap);
}
void orbx_launch_undistort(hipStream_t s, int B, int max_n, int cap, const double *K4, const double *k14, int identity,
                           const orbx_keypoint *kps, const int *counts, orbx_keypoint *out) {
    if (B <= 0 || max_n <= 0) return;
    DUndist u;
    u.fx = K4[0]; u.fy = K4[1]; u.cx = K4[2]; u.cy = K4[3];
    for (int i = 0; i < 14; ++i) u.k[i] = k14[i];
    u.identity = identity;
    hipLaunchKernelGGL(k_undistort, dim3((max_n + 255) / 256, B), dim3(256), 0, s, u, kps, counts, max_n, cap, out);
}
void orbx_launch_rgbd(hipStream_t s, int B, int max_n, int cap, const double *K4, const double *k14, int identity,
                      const OrbxRgbdArgs &a, const orbx_keypoint *kps, const orbx_keypoint *kun_in, const int *counts,
                      orbx_keypoint *kun_out, float *u_right, float *depth) {
    if (B <= 0 || max_n <= 0) return;
    DUndist u;
    u.fx = K4[0]; u.fy = K4[1]; u.cx = K4[2]; u.cy = K4[3];
    for (int i = 0; i < 14; ++i) u.k[i] = k14[i];
    u.identity = identity;
    DRgbd r;
    r.depth = a.depth; r.frame_stride = a.frame_stride; r.stride = a.stride; r.W = a.width;
    r.u16 = a.format == ORBX_DEPTH_U16;
    r.pitch = r.u16 ? 4LL * a.width : a.stride;
    r.limit = (long long)(a.height - 1) * r.pitch + 4LL * a.width;
    r.scale_rows = a.scale_f32; r.scale = a.scale; r.mbf = a.mbf;
    hipLaunchKernelGGL(k_rgbd, dim3((max_n + 255) / 256, B), dim3(256), 0, s, u, r, kps, kun_in, counts, max_n, cap, kun_out,
                       u_right, depth);
}
void orbx_launch_bow_transform(hipStream_t s, int B, int max_n, const int *child_begin, const uint32_t *child_ids,
                               const uint8_t *node_desc, int n_nodes, int L, const uint8_t *desc, const int *counts,
                               long long frame_stride, int levelsup, uint32_t *out_leaf, uint32_t *out_nid, int out_stride) {
    if (B <= 0 || max_n <= 0) return;
    DVoc v;
    v.child_begin = child_begin; v.child_ids = child_ids; v.desc = node_desc; v.n_nodes = n_nodes; v.L = L;
    hipLaunchKernelGGL(k_bow_transform, dim3((max_n + 15) / 16, B), dim3(256), 0, s, v, desc, counts, frame_stride, levelsup,
                       out_leaf, out_nid, out_stride);
}
static int g_qt_cus = 0;   // CUs of the current device (orbx_quadtree_prepare)
void orbx_launch_quadtree(hipStream_t s, const DGeom &g, int B, const uint2 *dense, const int *cand_count, uint32_t *lvl_kp, int *lvl_count,
                          int *status, uint16_t *knode_glob, int ncap, int lds_keys, int reg_keys, int level_begin, int level_count) {
    if (level_count <= 0) return;
    reg_keys = reg_keys < 0 ? 0 : reg_keys > QT_KPT ? QT_KPT : reg_keys;
    const size_t smem = orbx_quadtree_smem(ncap, lds_keys);
    // workgroups per CU of this launch decide the workgroup size (see k_quadtree)
    static int forced = -1;
    if (forced < 0) { const char *e = getenv("ORBX_QT_THREADS"); forced = e ? atoi(e) : 0; }
    const long long wgs = (long long)B * level_count, cus = g_qt_cus > 0 ? g_qt_cus : 256;
    int nfeat = 0;   // keys per workgroup scale with the feature quota: 2000 features want 512 threads even at 4 workgroups per CU
    for (int l = 0; l < g.nlevels; ++l) nfeat += g.lv[l].nfeat;   // (1241x376 / 2000, 128 frames: 77 / 63 / 99 us with 256 / 512 / 1024)
    int threads = wgs >= 4 * cus && nfeat <= 1600 ? 256 : wgs >= 2 * cus ? 512 : 1024;
    if (forced == 256 || forced == 512 || forced == 1024) threads = forced;
    const dim3 grid(B, level_count);   // frame fastest (see qt_workgroup)
    if (threads == 256)
        hipLaunchKernelGGL(k_quadtree<256>, grid, dim3(256), smem, s, g, dense, cand_count, lvl_kp, lvl_count, status, knode_glob, ncap, lds_keys, reg_keys, level_begin);
    else if (threads == 512)
        hipLaunchKernelGGL(k_quadtree<512>, grid, dim3(512), smem, s, g, dense, cand_count, lvl_kp, lvl_count, status, knode_glob, ncap, lds_keys, reg_keys, level_begin);
    else
        hipLaunchKernelGGL(k_quadtree<1024>, grid, dim3(1024), smem, s, g, dense, cand_count, lvl_kp, lvl_count, status, knode_glob, ncap, lds_keys, reg_keys, level_begin);
}
hipError_t orbx_quadtree_prepare(size_t smem) {
    // The attribute belongs to (function, device), not to a handle: ORB-SLAM2 itself keeps mpIniORBextractor (2 x nFeatures)
    // alive next to mpORBextractorLeft (src/Tracking.cc:171-182), so a later, smaller handle must never lower it.
    static std::mutex mu;
    static size_t cur[64] = {0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    if (g_qt_cus == 0) { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, dev) == hipSuccess) g_qt_cus = pr.multiProcessorCount; }
    if (dev >= 0 && dev < 64 && smem <= cur[dev]) return hipSuccess;
    e = hipFuncSetAttribute((const void *)k_quadtree<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_quadtree<512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_quadtree<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e == hipSuccess && dev >= 0 && dev < 64) cur[dev] = smem;
    return e;
}
void orbx_launch_blur(hipStream_t s, const DGeom &g, int B, const uint8_t *pyr, uint8_t *blur) {
    hipLaunchKernelGGL(k_blur, dim3(g.blur_tiles, B), dim3(256), 0, s, g, pyr, blur);
}
void orbx_launch_describe(hipStream_t s, const DGeom &g, int B, const uint8_t *pyr, const uint32_t *lvl_kp,
                          const int *lvl_count, float *lvl_angle, orbx_keypoint *kps, uint8_t *desc,
                          int *counts, int *status, int cap, const OrbxRaw0 *raw) {
#ifdef ORBX_TIMING_KNOBS
    static int dbg_stop = -1;
    if (dbg_stop < 0) { const char *e = getenv("ORBX_DESC_STOP"); dbg_stop = e ? atoi(e) : 0; }
#else
    const int dbg_stop = 0;
#endif
    const dim3 grid(8 * ((g.kp_total + DS_WPB - 1) / DS_WPB), (B + 7) / 8);
    const OrbxRaw0 none{nullptr, 0, 0, 0, 0};
    if (raw && g.fp_mode == ORBX_FP_GCC_FMA)
        hipLaunchKernelGGL((k_describe<ORBX_FP_GCC_FMA, true>), grid, dim3(64 * DS_WPB), 0, s, g, pyr, lvl_kp, lvl_count, lvl_angle, kps, desc, counts, status, cap, dbg_stop, B, *raw);
    else if (raw)
        hipLaunchKernelGGL((k_describe<ORBX_FP_STRICT, true>), grid, dim3(64 * DS_WPB), 0, s, g, pyr, lvl_kp, lvl_count, lvl_angle, kps, desc, counts, status, cap, dbg_stop, B, *raw);
    else if (g.fp_mode == ORBX_FP_GCC_FMA)
        hipLaunchKernelGGL((k_describe<ORBX_FP_GCC_FMA, false>), grid, dim3(64 * DS_WPB), 0, s, g, pyr, lvl_kp, lvl_count, lvl_angle, kps, desc, counts, status, cap, dbg_stop, B, none);
    else
        hipLaunchKernelGGL((k_describe<ORBX_FP_STRICT, false>), grid, dim3(64 * DS_WPB), 0, s, g, pyr, lvl_kp, lvl_count, lvl_angle, kps, desc, counts, status, cap, dbg_stop, B, none);
}
void orbx_launch_grid_build(hipStream_t s, const DGrid &gp, int nframes, const orbx_keypoint *kps, const int *counts, int fixed_n,
                            int cap, int *cell_begin, uint16_t *items) {
    if (nframes <= 0) return;
    hipLaunchKernelGGL(k_grid_build, dim3(nframes), dim3(1024), 0, s, gp, kps, counts, fixed_n, cap, cell_begin, items);
}
void orbx_launch_gate(hipStream_t s, const DGrid &gp, const orbx_keypoint *kps, const uint8_t *desc, const int *cell_begin,
                      const uint16_t *items, const DGateQuery *q, const uint8_t *qdesc, int nq, uint2 *span, uint32_t *cursor,
                      uint32_t *out_items, uint32_t cap, int fstride) {
    if (nq <= 0) return;
    hipLaunchKernelGGL(k_gate, dim3((nq + 3) / 4), dim3(256), 0, s, gp, kps, desc, cell_begin, items, q, qdesc, nq, span, cursor,
                       out_items, cap, fstride);
}
void orbx_launch_track_project(hipStream_t s, const OrbxTrackFrames &F, const float *camera4, float mbf, int fma_mode,
                               const DTrackProb *probs, DTrackQ *q, int nq) {
    if (nq <= 0) return;
    const DTrackCam cam = {camera4[0], camera4[1], camera4[2], camera4[3], F.bounds[0], F.bounds[1], F.bounds[2], F.bounds[3], mbf, fma_mode};
    hipLaunchKernelGGL(k_track_project, dim3((nq + 255) / 256), dim3(256), 0, s, cam, probs, q, nq);
}
void orbx_launch_track_frustum(hipStream_t s, const OrbxTrackFrames &F, const float *camera4, float mbf, int fma_mode, int nlevels,
                               const float *thr, const float *scale, int nproblems, int max_points, const DTrackProb *probs,
                               const DTrackLocal *locals, const DTrackPoolPt *pool, const uint8_t *pdesc, const int32_t *index,
                               const uint8_t *skip, DTrackQ *q, uint8_t *qdesc, uint8_t *in_view, orbx_track_state *track) {
    if (nproblems <= 0 || max_points <= 0) return;
    DTrackFrustumArgs A;
    A.cam = {camera4[0], camera4[1], camera4[2], camera4[3], F.bounds[0], F.bounds[1], F.bounds[2], F.bounds[3], mbf, fma_mode};
    A.nlevels = nlevels;
    for (int l = 0; l < ORBX_PS_LEVELS; ++l) { A.thr[l] = thr[l]; A.scale[l] = l < nlevels ? scale[l] : 0.f; }
    for (int p0 = 0; p0 < nproblems; p0 += 65535)   // the y extent of a grid
        hipLaunchKernelGGL(k_track_frustum, dim3((max_points + 255) / 256, std::min(65535, nproblems - p0)), dim3(256), 0, s, A, p0,
                           probs, locals, pool, pdesc, index, skip, q, qdesc, in_view, track);
}
void orbx_launch_track_cand(hipStream_t s, bool two, const OrbxTrackFrames &F, const DTrackProb *probs, const DTrackQ *q,
                            const uint8_t *qdesc, int nq, uint4 *cand) {
    if (nq <= 0) return;
    if (two) hipLaunchKernelGGL(k_track_cand<true>, dim3((nq + 3) / 4), dim3(256), 0, s, F.gp, probs, q, qdesc, nq, F.kps, F.desc, F.ur, F.counts, F.cap, F.cell_begin, F.items, cand);
    else hipLaunchKernelGGL(k_track_cand<false>, dim3((nq + 3) / 4), dim3(256), 0, s, F.gp, probs, q, qdesc, nq, F.kps, F.desc, F.ur, F.counts, F.cap, F.cell_begin, F.items, cand);
}
void orbx_launch_track_select(hipStream_t s, bool mp, const OrbxTrackFrames &F, int nproblems, const DTrackProb *probs, const DTrackQ *q,
                              const uint8_t *qdesc, const uint4 *cand, const uint32_t *seed, float nnratio, int check, int32_t *ev,
                              int32_t *out, int32_t *nmatches) {
    if (nproblems <= 0) return;
    const int words = (F.cap + 31) / 32;
    const size_t smem = ((size_t)words + 32) * sizeof(uint32_t);   // blocked bitmap | histogram; cap <= 65535: at most 8.1 KB
    if (mp) hipLaunchKernelGGL(k_track_select<true>, dim3(nproblems), dim3(64), smem, s, F.gp, probs, q, qdesc, cand, seed, words, F.kps, F.desc, F.ur, F.counts, F.cap, F.cell_begin, F.items, nnratio, check, ev, out, nmatches);
    else hipLaunchKernelGGL(k_track_select<false>, dim3(nproblems), dim3(64), smem, s, F.gp, probs, q, qdesc, cand, seed, words, F.kps, F.desc, F.ur, F.counts, F.cap, F.cell_begin, F.items, nnratio, check, ev, out, nmatches);
}
void orbx_launch_block_dist(hipStream_t s, const uint8_t *d1, const uint8_t *d2, const DDistRow *rows, const uint32_t *col_idx,
                            int nrows, uint16_t *out) {
    if (nrows <= 0) return;
    hipLaunchKernelGGL(k_block_dist, dim3((nrows + 3) / 4), dim3(256), 0, s, d1, d2, rows, col_idx, nrows, out);
}
void orbx_launch_bow_select(hipStream_t s, bool kk, const DBowItem *items, int nitems, const uint32_t *idx, const uint8_t *desc,
                            const uint8_t *hmp, float nnratio, int words, int32_t *out) {
    if (nitems <= 0) return;
    const size_t smem = (size_t)4 * words * sizeof(uint32_t);
    if (kk) hipLaunchKernelGGL(k_bow_select<true>, dim3((nitems + 3) / 4), dim3(256), smem, s, items, nitems, idx, desc, hmp, nnratio, words, out);
    else hipLaunchKernelGGL(k_bow_select<false>, dim3((nitems + 3) / 4), dim3(256), smem, s, items, nitems, idx, desc, hmp, nnratio, words, out);
}
void orbx_launch_bow_rot(hipStream_t s, bool kk, int nproblems, int nout, const uint32_t *cand_base, const float *ang, int check,
                         int32_t *out, int32_t *counts) {
    if (nproblems <= 0) return;
    if (kk) hipLaunchKernelGGL(k_bow_rot<true>, dim3(nproblems), dim3(BOW_ROT_THREADS), 0, s, nout, cand_base, ang, check, out, counts);
    else hipLaunchKernelGGL(k_bow_rot<false>, dim3(nproblems), dim3(BOW_ROT_THREADS), 0, s, nout, cand_base, ang, check, out, counts);
}
size_t orbx_match_workspace_bytes(int npairs, int out_stride) { return (size_t)npairs * MT_SPLIT * out_stride * sizeof(uint2); }
void orbx_launch_match(hipStream_t s, int npairs, int max_nq, const uint8_t *q, const int *nq, long long q_stride,
                       const uint8_t *t, const int *nt, long long t_stride, int *best_idx, int *best_dist,
                       int *second_dist, int out_stride, void *workspace, int kernel) {
    // kernel: 0 = matrix pipe, FP4 operands (default); 1 = vector pipe (ORBX_MATCH_KERNEL=valu); 2 = matrix pipe, int8 operands (=i8)
    const bool f4 = kernel == 0;
    if (npairs <= 0 || max_nq <= 0) return;
    const OrbxMatchPlan plan = orbx_match_plan(npairs, max_nq, kernel);   // QT and the train split (orbx_launch.h)
    const int nsplit = plan.nsplit;
    if (plan.qt == 0) {   // the vector-pipe kernel (orbx_params-free A/B switch ORBX_MATCH_KERNEL=valu, read once per handle)
        const int qblocks = (max_nq + 127) / 128;
        hipLaunchKernelGGL(k_match_valu, dim3(qblocks, nsplit, npairs), dim3(64), 0, s, q, nq, q_stride, t, nt, t_stride,
                           (uint2 *)workspace, out_stride, nsplit);
        hipLaunchKernelGGL(k_match_merge, dim3((max_nq + 255) / 256, npairs), dim3(256), 0, s, nq, (const uint2 *)workspace,
                           best_idx, best_dist, second_dist, out_stride, nsplit);
        return;
    }
    if (plan.qt == 4) {
        hipLaunchKernelGGL(f4 ? k_match_f4<4> : k_match<4>, dim3((max_nq + MT_QPB(4) - 1) / MT_QPB(4), 1, npairs), dim3(64 * MT_WAVES), 0, s, q, nq,
                           q_stride, t, nt, t_stride, (uint2 *)workspace, best_idx, best_dist, second_dist, out_stride, 1);
        return;
    }
    const int qblocks = (max_nq + MT_QPB(2) - 1) / MT_QPB(2);
    hipLaunchKernelGGL(f4 ? k_match_f4<2> : k_match<2>, dim3(qblocks, nsplit, npairs), dim3(64 * MT_WAVES), 0, s, q, nq,
                       q_stride, t, nt, t_stride, (uint2 *)workspace, best_idx, best_dist, second_dist, out_stride, nsplit);
    if (nsplit > 1)
        hipLaunchKernelGGL(k_match_merge, dim3((max_nq + 255) / 256, npairs), dim3(256), 0, s, nq, (const uint2 *)workspace,
                           best_idx, best_dist, second_dist, out_stride, nsplit);
}
void orbx_launch_hamming_matrix(hipStream_t s, const uint8_t *q, int nq, const uint8_t *t, int nt, uint16_t *dist) {
    const long long n = (long long)nq * nt;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_hamming_matrix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, q, nq, t, nt, dist);
}

int orbx_stereo_items_per_pair(const OrbxStereoGeom &sg, int cap) {
    float smax = 1.f;
    for (int l = 0; l < sg.nlevels; ++l) smax = sg.scale[l] > smax ? sg.scale[l] : smax;
    return cap * (2 * (int)ceilf(2.0f * smax) + 3);
}
void orbx_launch_stereo_batch(hipStream_t s, const OrbxStereoGeom &sg, int npairs, int cap, const orbx_keypoint *kL,
                              const uint8_t *dL, const int *nL, const orbx_keypoint *kR, const uint8_t *dR, const int *nR,
                              const uint8_t *pyrL, const uint8_t *pyrR, long long pyr_bytes, float *uRight, float *depth,
                              int *sad, int *nmatches, int *row_begin, uint2 *row_items) {
    if (npairs <= 0 || cap <= 0) return;
    const int ipp = orbx_stereo_items_per_pair(sg, cap);
    const bool table = row_begin && row_items && sg.nrows0 <= ST_MAX_ROWS;
    if (table) hipLaunchKernelGGL(k_stereo_rows, dim3(npairs), dim3(1024), 0, s, sg, kR, nR, cap, row_begin, row_items, ipp, 0);
    hipLaunchKernelGGL(k_stereo_batch, dim3((cap + ST_KPB - 1) / ST_KPB, npairs), dim3(256), 0, s, sg, kL, dL, nL, kR, dR, nR, cap, pyrL, pyrR,
                       pyr_bytes, uRight, depth, sad, table ? row_begin : nullptr, table ? row_items : nullptr, ipp);
    hipLaunchKernelGGL(k_stereo_cut, dim3(npairs), dim3(256), 0, s, nL, cap, sad, uRight, depth, nmatches);
}
void orbx_launch_stereo(hipStream_t s, const OrbxStereoGeom &sg, const orbx_keypoint *kL, const uint8_t *dL, int nL,
                        const orbx_keypoint *kR, const uint8_t *dR, int nR, const uint8_t *pyrL, const uint8_t *pyrR,
                        float *uRight, float *depth, int *sad, int *row_begin, uint2 *row_items) {
    if (nL <= 0) return;
    // the row table of the batched form (vRowIndices) for the one pair too: without it a left keypoint's 16 lanes walk every
    // right keypoint
    const bool table = row_begin && row_items && sg.nrows0 <= ST_MAX_ROWS && nR > 0;
    if (table)
        hipLaunchKernelGGL(k_stereo_rows, dim3(1), dim3(1024), 0, s, sg, kR, (const int *)nullptr, nR, row_begin, row_items,
                           orbx_stereo_items_per_pair(sg, nR), nR);
    hipLaunchKernelGGL(k_stereo, dim3((nL + ST_KPB - 1) / ST_KPB), dim3(256), 0, s, sg, kL, dL, nL, kR, dR, nR, pyrL, pyrR, uRight,
                       depth, sad, table ? row_begin : nullptr, table ? row_items : nullptr);
}
void orbx_launch_kfdb_common(hipStream_t s, const uint2 *slots, int nslots, const uint32_t *pool_w, const uint32_t *qw_all,
                             const int *q_begin, int q0, int nq, const uint8_t *connected, int *qmax, uint32_t *cursor,
                             DKfRec *rec, uint32_t cap) {
    if (nslots <= 0 || nq <= 0) return;
    // every workgroup stages its query once: enough entries per workgroup to pay for that, enough workgroups to fill the device
    // and few enough waves that each appends its records in batches (64 entries per wave once the device is full)
    const int fill = (2048 + nq - 1) / nq, most = (nslots + 3) / 4;
    int gx = (nslots + 255) / 256;
    if (gx < (fill < most ? fill : most)) gx = fill < most ? fill : most;
    hipLaunchKernelGGL(k_kfdb_common, dim3(gx, nq), dim3(256), 0, s, slots, nslots, pool_w, qw_all, q_begin, q0, connected, qmax,
                       cursor, rec, cap);
}
void orbx_launch_kfdb_score(hipStream_t s, DKfRec *rec, const uint32_t *cursor, uint32_t cap, const int *qmax, const uint2 *slots,
                            const uint32_t *pool_w, const double *pool_v, const uint32_t *qw_all, const double *qv_all,
                            const int *q_begin, int scoring, int fma_mode) {
    if (cap == 0) return;
    unsigned g = (cap + 3) / 4;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(k_kfdb_score, dim3(g), dim3(256), 0, s, rec, cursor, cap, qmax, slots, pool_w, pool_v, qw_all, qv_all,
                       q_begin, scoring, fma_mode);
}
void orbx_launch_kfdb_score_slots(hipStream_t s, const uint32_t *slot_list, int n, const uint2 *slots, const uint32_t *pool_w,
                                  const double *pool_v, const uint32_t *qw, const double *qv, int nq, int scoring, int fma_mode,
                                  double *out) {
    if (n <= 0) return;
    int g = (n + 3) / 4;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(k_kfdb_score_slots, dim3(g), dim3(256), 0, s, slot_list, n, slots, pool_w, pool_v, qw, qv, nq, scoring,
                       fma_mode, out);
}
void orbx_launch_mp_distinct(hipStream_t s, const int32_t *obs_begin, const uint8_t *desc, const int64_t *obs_row,
                             const int32_t *order, int n_small, int n_wide, int32_t *best_idx, int32_t *best_median,
                             uint8_t *best_desc) {
    DMpDistinct A = {obs_begin, desc, obs_row, order, n_small, best_idx, best_median, (uint4 *)best_desc};
    const int per_block = 256 / ORBX_MP_GROUP;
    if (n_small > 0) hipLaunchKernelGGL(k_mp_distinct, dim3((n_small + per_block - 1) / per_block), dim3(256), 0, s, A);
    A.order = order + n_small; A.count = n_wide;
    if (n_wide > 0) hipLaunchKernelGGL(k_mp_distinct_wide, dim3(n_wide), dim3(256), 0, s, A);
}
void orbx_launch_mp_normal_depth(hipStream_t s, const int32_t *obs_begin, const DMpPoint *pts, const float *centers, int npoints,
                                 float scale_last, float *out) {
    if (npoints <= 0) return;
    hipLaunchKernelGGL(k_mp_normal_depth, dim3((npoints + 15) / 16), dim3(256), 0, s, obs_begin, pts, centers, npoints, scale_last, out);
}
void orbx_launch_pose_opt(hipStream_t s, const DPoseArgs &a) {
    if (a.nproblems <= 0) return;
    hipLaunchKernelGGL(k_pose_opt, dim3(a.nproblems), dim3(64), 0, s, a);
}
void orbx_launch_local_ba(hipStream_t s, const DLbaArgs &a) {
    if (a.nproblems <= 0) return;
    hipLaunchKernelGGL(k_local_ba, dim3(a.nproblems), dim3(ORBX_LBA_THREADS), 0, s, a);
}
void orbx_launch_essential_graph(hipStream_t s, const DEgArgs &a) {
    if (a.nproblems <= 0) return;
    hipLaunchKernelGGL(k_essential_graph, dim3(a.nproblems), dim3(ORBX_EG_THREADS), 0, s, a);
    if (a.npoints > 0) hipLaunchKernelGGL(k_eg_correct_points, dim3((unsigned)((a.npoints + 255) / 256)), dim3(256), 0, s, a);
}
void orbx_launch_sim3_opt(hipStream_t s, const DSim3OptArgs &a) {
    if (a.nproblems <= 0) return;
    hipLaunchKernelGGL(k_sim3_opt, dim3(a.nproblems), dim3(64), 0, s, a);
}
void orbx_launch_sim3(hipStream_t s, const DSim3Args &a) {
    if (a.total_hyps <= 0 || a.ngroups <= 0) return;
    hipLaunchKernelGGL(k_sim3_hypotheses, dim3((a.total_hyps + 63) / 64), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_sim3_inliers, dim3(a.ngroups), dim3(64 * ORBX_SIM3_WAVES), 0, s, a);
}
void orbx_launch_pnp(hipStream_t s, const DPnpArgs &a) {
    if (a.total_hyps <= 0 || a.ngroups <= 0) return;
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3((a.total_hyps + ORBX_PNP_HYP_LANES - 1) / ORBX_PNP_HYP_LANES), dim3(ORBX_PNP_HYP_LANES),
                       0, s, a);
    hipLaunchKernelGGL(k_pnp_inliers, dim3(a.ngroups), dim3(64 * ORBX_PNP_WAVES), 0, s, a);
}
void orbx_launch_init(hipStream_t s, const DInitArgs &a) {
    if (a.total_hyps <= 0 || a.ngroups <= 0) return;
    hipLaunchKernelGGL(k_init_hypotheses, dim3((a.total_hyps + ORBX_INIT_HYP_LANES - 1) / ORBX_INIT_HYP_LANES),
                       dim3(ORBX_INIT_HYP_LANES), 0, s, a);
    hipLaunchKernelGGL(k_init_scores, dim3(a.ngroups), dim3(ORBX_INIT_SCORE_LANES), 0, s, a);
}
void orbx_launch_recon(hipStream_t s, const DReconArgs &a) {
    if (a.nlaunch <= 0) return;
    hipLaunchKernelGGL(k_init_decompose, dim3((a.nlaunch + ORBX_RECON_LANES - 1) / ORBX_RECON_LANES), dim3(ORBX_RECON_LANES), 0, s, a);
    hipLaunchKernelGGL(k_init_check_rt, dim3(a.nlaunch * ORBX_RECON_MAX_HYP), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_init_pick, dim3(a.nlaunch), dim3(64), 0, s, a);
}
void orbx_launch_init_select(hipStream_t s, const DInitArgs &i, const DReconArgs &a) {
    if (a.nlaunch <= 0) return;
    hipLaunchKernelGGL(k_init_select, dim3(a.nlaunch), dim3(64), 0, s, i, a);
}
void orbx_launch_new_points(hipStream_t s, const DNewPtsArgs &a) {
    if (a.nchunks <= 0) return;
    hipLaunchKernelGGL(k_new_points, dim3(a.nchunks), dim3(ORBX_NEWPTS_CHUNK), 0, s, a);
}
void orbx_launch_sim3_search(hipStream_t s, const DSim3sArgs &a, const OrbxSim3sGrid &g) {
    if (a.nq <= 0 || a.nproblems <= 0) return;
    const DGrid gp = {g.minx, g.miny, g.winv, g.hinv};
    const int bx = (a.max_n + 255) / 256;
    hipLaunchKernelGGL(k_grid_build, dim3(a.nkf), dim3(1024), 0, s, gp, a.keys, a.cnt, 0, a.fstride, a.cb, a.items);
    hipLaunchKernelGGL(k_sim3s_project, dim3(bx, 2 * a.nproblems), dim3(256), 0, s, a);
    // one wave per live query up to 2048 workgroups; the waves stride over the rest
    hipLaunchKernelGGL(k_sim3s_cand, dim3(std::min((a.nq + 3) / 4, 2048)), dim3(256), 0, s, a, gp);
    hipLaunchKernelGGL(k_sim3s_mutual, dim3(bx, a.nproblems), dim3(256), 0, s, a);
}
