/* orbx_rect_digest.h -- the host-side digest of cv::remap's float maps (OpenCV 3.2 imgproc/imgwarp.cpp, INTER_LINEAR with
 * CV_32FC1 maps), shared by the library (orbx_set_rectification, orbx_debug_rect_digest) and the CPU oracle
 * (orc_remap_linear_u8).  Plain C99 / C++, no HIP: tests/san_rect_digest.cpp compiles it alone.
 *
 *   s  = cvRound(map * 32)                      INTER_TAB_SIZE = 32, half to even, a 32-BIT conversion
 *   i  = saturate_cast<short>(s >> 5)           arithmetic shift
 *   f  = s & 31
 *
 * cvRound is cvtss2si / _mm_cvtps_epi32 on x86: NaN, +-inf and every value outside [-2^31, 2^31) convert to the "integer
 * indefinite" INT_MIN.  (int)lrintf(v) is NOT that: lrintf returns a 64-bit long and the cast wraps, so NaN, +-inf and +-2^27
 * (times 32 = 2^32) came out as 0 -- column / row 0 with fraction 0, a real pixel of the raw image -- where OpenCV gets
 * i = -32768 and writes the border value.  Hence the range test below. */
#ifndef ORBX_RECT_DIGEST_H
#define ORBX_RECT_DIGEST_H
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

/* cvRound(float) as OpenCV 3.2 compiles it on x86-64: half to even, INT_MIN for NaN and anything not in [-2^31, 2^31).
 * (A float below 2^31 is at most 2^31 - 128, so lrintf of a value that passes the test fits an int.) */
static inline int orbx_cv_round32(float v) {
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return INT_MIN;
    return (int)lrintf(v);
}

/* one map entry: *xy = ix | iy << 16 (int16 each), *frac = fy << 5 | fx -- what k_pyr_l0_remap reads */
static inline void orbx_rect_digest_entry(float map_x, float map_y, uint32_t *xy, uint32_t *frac) {
    const int sx = orbx_cv_round32(map_x * 32.f), sy = orbx_cv_round32(map_y * 32.f);
    const int qx = sx >> 5, qy = sy >> 5;
    const int ix = qx < -32768 ? -32768 : qx > 32767 ? 32767 : qx, iy = qy < -32768 ? -32768 : qy > 32767 ? 32767 : qy;
    *xy = (uint32_t)(uint16_t)(int16_t)ix | ((uint32_t)(uint16_t)(int16_t)iy << 16);
    *frac = (uint32_t)(((sy & 31) << 5) | (sx & 31));
}

/* n entries; out_xy / out_frac may be the two halves of an interleaved array: entry i is written at [i * out_step] */
static inline void orbx_rect_digest(const float *map_x, const float *map_y, size_t n, uint32_t *out_xy, uint32_t *out_frac,
                                    size_t out_step) {
    for (size_t i = 0; i < n; ++i) orbx_rect_digest_entry(map_x[i], map_y[i], out_xy + i * out_step, out_frac + i * out_step);
}
#endif
