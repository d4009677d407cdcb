// orbx_inplace.h -- address arithmetic of the kernels that read level 0 IN PLACE from the caller's grey image
// (k_pyr_resize_rows_l1, k_fast_rows_ip, k_describe<., true>) instead of from the padded copy k_pyr_l0 writes.
//
// Invariant: no load of those kernels touches a byte outside [frame base, frame base + (H - 1) * stride + W) of its own frame,
// lanes whose data is discarded included.  Every load below is in fact kept inside its own ROW, [row * stride, row * stride + W).
// The helpers are __host__ __device__ so that tests/san_level0.cpp walks the very same arithmetic on the CPU.
//
// Padded coordinate P of level 0 holds raw pixel reflect101(P - 19, n); a patch that leaves the padded image itself reads
// reflect101(P, pn) of it (k_describe's edge path), so the composed map is reflect101(reflect101(P, pn) - 19, n).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ORBX_IP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define ORBX_IP_FN inline
#endif

#define ORBX_IP_EDGE 19        // == ORBX_EDGE
#define ORBX_IP_MIN_W 64       // smallest image the in-place mode takes: k_describe's edge window is 48 bytes of one row, the
#define ORBX_IP_MIN_H 64       // clamped FAST pieces 12, the level-1 tail window 8; 64 keeps every reflection a single one
// Input lifetime.  With the eager copy only the FIRST kernel of a call reads the caller's image; in place, the image is read until
// the call's last kernel (k_describe) has finished on the handle's stream, and must stay valid and unchanged until then
// (include/orbx.h).  The Python wrapper keeps a reference to the input of the last device call for that reason.
#define ORBX_IP_DS_WIN 48      // bytes of a source row k_describe loads per patch row (4 lanes x 12)
#define ORBX_IP_DS_W 43        // patch width / height (DS_W)

// the caller's image as the kernels see it
struct OrbxRaw0 {
    const uint8_t *img;        // frame 0
    long long frame_stride;    // bytes between frames
    int W, H, stride;
};

ORBX_IP_FN int orbx_ip_reflect(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}
// raw coordinate of padded coordinate P (any P the kernels form: the padded image may be left by a few pixels)
ORBX_IP_FN int orbx_ip_map(int P, int n) { return orbx_ip_reflect(orbx_ip_reflect(P, n + 2 * ORBX_IP_EDGE) - ORBX_IP_EDGE, n); }

// ---- k_pyr_resize_rows_l1: a lane needs the bytes [lo, hi] of a source row, hi - lo <= 7 (checked on the host).
// Body strips read the dword-aligned 12-byte window around them; a strip with a lane whose window would leave the row is a
// TAIL strip: its lanes read 8 bytes from `org` = min(lo, W - 8) at byte alignment.
ORBX_IP_FN bool orbx_ip_rr_window_leaves_row(int lo, int W) { return (lo & ~3) + 12 > W; }
ORBX_IP_FN int orbx_ip_rr_body_col(int lo) { return lo & ~3; }                 // 12 bytes from here
ORBX_IP_FN int orbx_ip_rr_tail_col(int lo, int W) { return lo < W - 8 ? lo : W - 8; }   // 8 bytes from here
ORBX_IP_FN uint32_t orbx_ip_row_off(int row, int stride, int col) { return (uint32_t)row * (uint32_t)stride + (uint32_t)col; }

// ---- k_fast_rows, level-0 groups.  The tile of a group starts at padded column x0 = raw column x0 - 19 (-3 for the first
// cell column) and is `tw` columns wide; lane piece dq (0..6) loads 12 bytes of a row.
//   xb  = raw column of LDS tile byte 4 * dsh (the first loaded byte): 0 for the first cell column (dsh = 1: the three ring
//         columns in front of it take LDS bytes 1..3), else the raw column of the tile origin rounded down to a dword
//   piece dq wants [xb + 12 dq, + 12); a piece that would leave the row is loaded from W - 12 and shifted right by the
//   difference in registers (bytes shifted in from beyond the row are ring or unused columns, mirrored in LDS afterwards)
ORBX_IP_FN int orbx_ip_fast_xb(int x0, int *dsh) {
    const int rs = x0 - ORBX_IP_EDGE;
    if (rs < 0) { *dsh = 1; return 0; }       // rs = -3: cells start at padded column 16.  With dsh = 1 LDS byte 0 of every tile row
                                              // is never written -- and never read: the tile starts at byte 1 (orbx_ip_fast_tile_off);
                                              // tests/san_level0.cpp compares every tile byte the kernel reads, so a read of it would show
    *dsh = 0;
    const int xb = rs & ~3;                   // dword-aligned in the RAW row (base and stride are multiples of 4): aligned 12-byte pieces
    return xb;
}
ORBX_IP_FN int orbx_ip_fast_tile_off(int x0) {   // LDS byte of padded column x0 inside a tile row
    int dsh;
    const int xb = orbx_ip_fast_xb(x0, &dsh);
    return x0 - ORBX_IP_EDGE - xb + 4 * dsh;
}
ORBX_IP_FN int orbx_ip_fast_piece_col(int xb, int dq, int W, int *shr) {
    const int col = xb + 12 * dq;
    const int over = col + 12 - W;
    *shr = over > 0 ? over : 0;
    return over > 0 ? W - 12 : col;
}
ORBX_IP_FN int orbx_ip_fast_row(int prow, int H) { return orbx_ip_reflect(prow - ORBX_IP_EDGE, H); }

// ---- k_describe, level-0 keypoints.  The 43 x 43 patch starts at raw (rx0, ry0) = padded (px0 - 19, py0 - 19).
// interior: the slab path's code on the raw image (dword-aligned 48-byte window inside the row, 43 rows inside the image).
// edge: patch row r comes from raw row orbx_ip_map(py0 + r, H); its 48-byte window starts at ws = clamp(rx0, 0, W - 48)
// (byte alignment) and is laid into the LDS row displaced by ws - rx0; the ring columns are then mirrored from the row itself.
ORBX_IP_FN bool orbx_ip_desc_interior(int rx0, int ry0, int W, int H) {
    return rx0 >= 0 && ry0 >= 0 && (rx0 & ~3) + ORBX_IP_DS_WIN <= W && ry0 + ORBX_IP_DS_W <= H;
}
ORBX_IP_FN int orbx_ip_desc_ws(int rx0, int W) { return rx0 < 0 ? 0 : (rx0 > W - ORBX_IP_DS_WIN ? W - ORBX_IP_DS_WIN : rx0); }
