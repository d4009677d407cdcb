// The FAST-9/16 corner test and cv::cornerScore of ONE candidate as one min / max network on the raw ring bytes.  Shared by the
// two instances of fr_round (k_fast_rows, orbx_kernels.hip) and by the host check tests/fast_net.cpp: plain C++, no HIP type.
//
// cv::FAST's test (9 contiguous ring pixels all brighter than v + th, or all darker than v - th) is "the largest over the 16 arcs
// of the smallest signed difference on the arc exceeds th", and that quantity is cv::cornerScore + 1.  Minimum and maximum commute
// with adding a constant and, swapped, with x -> 255 - x, so the network runs on y = ring ^ m (m = 0: brighter, m = 0xffff: darker
// = the complemented bytes, 0xff00 + 255 - x as a 16-bit value) and the centre is subtracted ONCE at the end:
//     margin = max over the arcs of (min over the arc's 9 pixels of y)  -  (v ^ m)
//     corner <=> margin > th          score = margin - 1
// One full-rate xor per ring pixel; no signed difference, no multiply-add, no sign bookkeeping.
//
// A 9-arc of the 16-ring is a suffix of one half of the ring (pixels 0..7 or 8..15) plus a prefix of the other half:
//     arc(8b + o) = min(S[b][o], P[1-b][o]),   P[b][o] = min(y[8b .. 8b+o]),   S[b][o] = min(y[8b+o .. 8b+7])
// The prefix and suffix minima of the two halves are 2 * (7 + 6) = 26 two-input minima (S[b][0] is P[b][7]), the arcs 16 more,
// the 16-way maximum 15: 57 operations, where doubling (m2, m4, m8, + the ninth pixel, + the maximum) takes 80.  Minimum and
// maximum are associative, so the result is the same integer for any data.  Every prefix / suffix value but S[b][1] has two uses
// (the next one of its chain and an arc), so the compiler has nothing to fuse into the quarter-rate three-input 16-bit forms there.
//
// Polarity: the compass pixels (ring 0 / 4 / 8 / 12) give the larger margin,
//     mb = min(max(x0, x8), max(x4, x12)) - v   (brighter)      md = v - max(min(x0, x8), min(x4, x12))   (darker)
// darker iff md > mb (a tie goes to brighter); `other` forces the opposite one (the re-run of a candidate that passed BOTH
// pre-tests, min(mb, md) > th, and failed the polarity taken first).  The differences stay within -510 .. 510: no 16-bit overflow
// for th <= 255, and a threshold of 0x4000 (a lane without an entry) is reached by nothing.
#ifndef ORBX_FAST_NET_H
#define ORBX_FAST_NET_H
#include <stdint.h>

#if defined(__HIPCC__)
#define ORBX_FN_HD __host__ __device__ __forceinline__
#else
#define ORBX_FN_HD inline
#endif

// Steering of the instruction selection (device code; the host computes the same integers).  gfx950 issues the three-input 16-bit
// forms v_min3_u16 / v_max3_u16 at a QUARTER of the rate of the two-input ones, and the compiler fuses min(min(a, b), c) into them
// wherever the inner value has one use and both operations have the same signedness.  All 16 values of one candidate lie in
// 0 .. 0xff (m = 0) or all in 0xff00 .. 0xffff (m = 0xffff), so signed and unsigned comparisons order them alike -- which the compiler
// cannot know, m being data.  The single-use values are therefore consumed by the operation of the OTHER signedness: no fence
// (an empty asm costs an `s_nop` each), no extra instruction.
// The 16-way maximum is a tree of two-input maxima, unsigned / signed level by level (15 operations).  (Seven 32-bit v_max3_u32
// + one v_max_u32 on the zero-extended values, written as inline asm, measured the same: profiles/fast_net.md.  Not kept.)

typedef unsigned short ofn_u16;
typedef short ofn_i16;
ORBX_FN_HD ofn_u16 ofn_min(ofn_u16 a, ofn_u16 b) { return a < b ? a : b; }
ORBX_FN_HD ofn_u16 ofn_max(ofn_u16 a, ofn_u16 b) { return a > b ? a : b; }
ORBX_FN_HD ofn_i16 ofn_smin(ofn_i16 a, ofn_i16 b) { return a < b ? a : b; }
ORBX_FN_HD ofn_i16 ofn_smax(ofn_i16 a, ofn_i16 b) { return a > b ? a : b; }
// the same value as ofn_min / ofn_max for two values of one candidate (see above)
ORBX_FN_HD ofn_u16 ofn_min_s(ofn_u16 a, ofn_u16 b) { return (ofn_u16)ofn_smin((ofn_i16)a, (ofn_i16)b); }
ORBX_FN_HD ofn_u16 ofn_max_s(ofn_u16 a, ofn_u16 b) { return (ofn_u16)ofn_smax((ofn_i16)a, (ofn_i16)b); }

// maximum of the 16 arc minima
ORBX_FN_HD ofn_u16 ofn_max16(const ofn_u16 (&a)[16]) {
    ofn_u16 t8[8], t4[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) t8[i] = ofn_max(a[2 * i], a[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 4; ++i) t4[i] = ofn_max_s(t8[2 * i], t8[2 * i + 1]);
    return ofn_max_s(ofn_max(t4[0], t4[1]), ofn_max(t4[2], t4[3]));
}

// v: the centre; x[k]: ring pixel k in the order of fr_round's ro[] table ((dx, dy) = (0, 3), (1, 3), (2, 2), (3, 1), (3, 0), ...:
// any order that walks the ring serves); th: the threshold, 0 .. 255, or 0x4000 for "no entry".
ORBX_FN_HD void orbx_fast_net(ofn_u16 v, const ofn_u16 (&x)[16], ofn_i16 th, bool other, bool &corner, uint8_t &score, bool &both) {
    const ofn_u16 hi = ofn_min(ofn_max(x[0], x[8]), ofn_max(x[4], x[12]));
    const ofn_u16 lo = ofn_max(ofn_min(x[0], x[8]), ofn_min(x[4], x[12]));
    const ofn_i16 mb = (ofn_i16)(hi - v), md = (ofn_i16)(v - lo);
    both = ofn_smin(mb, md) > th;
    // (a compare, an `s_nop 1` for the mask hazard and a select; the sign of mb - md by subtract-and-shift compiles to the same)
    const ofn_u16 m = (md > mb) != other ? (ofn_u16)0xffff : (ofn_u16)0;
    ofn_u16 y[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) y[k] = (ofn_u16)(x[k] ^ m);
    ofn_u16 P[2][8], S[2][8], a[16];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        P[b][0] = y[8 * b];
#pragma unroll
        for (int o = 1; o < 8; ++o) P[b][o] = ofn_min(P[b][o - 1], y[8 * b + o]);
        S[b][7] = y[8 * b + 7];
#pragma unroll
        for (int o = 6; o >= 1; --o) S[b][o] = ofn_min(S[b][o + 1], y[8 * b + o]);
        S[b][0] = P[b][7];
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int o = 0; o < 8; ++o) a[8 * b + o] = o == 1 ? ofn_min_s(S[b][o], P[1 - b][o]) : ofn_min(S[b][o], P[1 - b][o]);   // S[b][1] has this one use
    }
    const ofn_i16 margin = (ofn_i16)(ofn_max16(a) - (ofn_u16)(v ^ m));
    corner = margin > th;
    score = (uint8_t)(margin - 1);
}
#endif
