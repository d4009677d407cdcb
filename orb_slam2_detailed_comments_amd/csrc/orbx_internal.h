// orbx_internal.h -- host-side geometry / workspace description shared by the API and kernels.
#pragma once
#include <cstdint>
#include <vector>
#include "../../include/orbx.h"

#define ORBX_MAX_LEVELS 16
#define ORBX_EDGE 19        // EDGE_THRESHOLD, reference src/ORBextractor.cc:82
#define ORBX_HALF_PATCH 15  // HALF_PATCH_SIZE, :81
#define ORBX_PATCH 31       // PATCH_SIZE, :80
#define ORBX_NPATCH 749     // pixels of the orientation disc defined by umax

// One FAST cell (reference src/ORBextractor.cc:1465-1503): sub-image [y0,y0+ch) x [x0,x0+cw) of the padded level.
struct OrbxCell {
    int16_t x0, y0, cw, ch;  // sub-mat origin and size (padded-level = slab coordinates; upstream: view coordinate + 19)
    int16_t offx, offy;      // j*wCell, i*hCell  (added to the sub-mat-local keypoint, :1540-1541)
    int16_t level;
    int16_t idx_in_level;    // row-major ordinal of the cell inside its level (emission order)
    int32_t slot_begin;      // first candidate slot of this cell inside its level's candidate region
    int32_t slot_cap;        // slots reserved: strict 3x3 maxima leave at most one survivor per 2x2 block
};

// One wave of k_fast_rows: `ncell` (1 or 2) horizontally adjacent cells of one cell row whose interiors together span
// at most 64 + ORBX_FAST_XCOLS columns (one lane per interior column in the row walk; the columns beyond the wave are tested
// apart, lanes as rows).  The LDS tile pitch of the kernel bounds it: 64 + XCOLS + 6 ring + 3 alignment bytes <= 76.
#define ORBX_FAST_XCOLS 2
struct OrbxFastGroup {
    int32_t cell0;
    int32_t ncell;
};
// Sub-batch pipeline of the batched extraction (orbx_extract.cpp run_chunk): the pyramid of sub-batch k+1 runs on the side stream
// next to FAST / quadtree / descriptors of sub-batch k.  k_fast_rows (96 VGPRs, one-wave workgroups) fills every CU with 5 waves
// per SIMD; with ORBX_FAST_ROOM=1 its LDS request is raised to ORBX_LDS_PER_CU / ORBX_FAST_PIPE_WAVES bytes, so a CU holds
// ORBX_FAST_PIPE_WAVES of its waves and 128 registers per lane stay free for the pyramid kernels (no LDS) on every SIMD
// (measured slower than letting the pyramid take the slots FAST waves free as they retire: off by default).
#define ORBX_LDS_PER_CU (160 * 1024)
#define ORBX_FAST_PIPE_WAVES 16
#define ORBX_PIPE_MAX 8            // most sub-batches per batch
#define ORBX_PIPE_MIN_FRAMES 256   // smaller batches keep the serial sequence
// Sub-batch offsets of a batch of B frames, shared by the sub-batch pipeline and the FAST-first plan of run_chunk: up to S
// sub-batches [off[k], off[k + 1]), off[0] = 0, off[n] = B; returns n (off holds ORBX_PIPE_MAX + 1 entries).  Every offset but
// the last is a multiple of 8 frames (k_describe deals frames over the 8 XCDs) and the last sub-batch takes the rest; `head`
// makes the first sub-batch half the size of the others.  No sub-batch is smaller than 8 frames: a batch too small for S of
// them gets fewer (one, below 16 frames).
static inline int orbx_split_batch(int B, int S, bool head, int *off) {
    S = S < 1 ? 1 : S > ORBX_PIPE_MAX ? ORBX_PIPE_MAX : S;
    const int units = head ? 2 * S - 1 : S;
    int n = 0;
    off[0] = 0;
    while (n + 1 < S) {
        const int share = (int)((long long)B * (head && n > 0 ? 2 : 1) / units) & ~7;
        const int next = off[n] + (share > 8 ? share : 8);
        if (B - next < 8) break;
        off[++n] = next;
    }
    off[++n] = B;
    return n;
}

// resize tap for one padded destination coordinate (border folded in by reflect-101)
struct OrbxTap {
    int16_t s0, s1;  // source index of the two taps (already clamped)
    int16_t a0, a1;  // 11-bit fixed-point weights
};

struct OrbxLevelGeom {
    int sw, sh;          // un-padded size
    int pw, ph, pitch;   // padded size and row pitch in bytes
    int org;             // where mvImagePyramid[level] starts inside the padded level: 0 (fork) or ORBX_EDGE (upstream), both axes
    int vw, vh;          // size of mvImagePyramid[level]: pw x ph (fork) or sw x sh (upstream)
    int64_t off;         // byte offset of this level inside one frame's pyramid slab
    int ncols, nrows, wcell, hcell;
    int cell_begin, cell_count;  // range in the per-frame cell table
    int qt_w, qt_h;      // quadtree region (maxBorder - minBorder)
    int nini;            // number of root nodes
    float hx;            // root width
    int nfeat;           // mnFeaturesPerLevel
    int kp_cap;          // max keypoints the quadtree can emit: max(nfeat + 3, 4 * nini)
    int kp_begin;        // slot offset inside the per-frame level-keypoint table
    int cand_cap;        // candidate slots
    int64_t cand_begin;  // offset inside the per-frame candidate table
    int tapx_begin, tapy_begin;  // offsets into the tap table (level > 0)
    bool narrow_taps;    // every aligned group of 4 destination columns reads <= 8 consecutive source bytes (k_pyr_resize_rows)
    float scale;         // mvScaleFactor[level]
    float size;          // (float)(int)(31 * scale)
};

struct OrbxGeom {
    int width = 0, height = 0, nlevels = 0;
    OrbxLevelGeom lv[ORBX_MAX_LEVELS];
    std::vector<OrbxCell> cells;
    std::vector<OrbxFastGroup> fast_groups;
    std::vector<OrbxTap> taps;
    int64_t pyr_bytes = 0;     // per frame
    int64_t cand_total = 0;    // per frame
    int kp_total = 0;          // per frame: sum of kp_cap
    int node_cap = 0;          // max over levels of quadtree node capacity
    int max_cand_cap = 0;
    // in-place mode (orbx_inplace.h): level 1 resized straight from the caller's grey image.  A second tap table for level 1
    // (lv[1].pw horizontal records, then lv[1].ph vertical ones, appended to `taps`) carries RAW source indices with level 0's
    // reflect-101 border folded in.  l1_inplace: the table passed the narrow-footprint check of k_pyr_resize_rows_l1 and the
    // image is large enough for the in-place paths of the three consumers; l1_tail_bx: first column strip of tail form.
    int l1_tap_begin = 0, l1_tail_bx = 0;
    bool l1_inplace = false;
};

struct OrbxTables {
    float scale[ORBX_MAX_LEVELS], inv_scale[ORBX_MAX_LEVELS], sigma2[ORBX_MAX_LEVELS], inv_sigma2[ORBX_MAX_LEVELS];
    int nfeat[ORBX_MAX_LEVELS];
    int umax[ORBX_HALF_PATCH + 1];
};

// host-only math (orbx_geometry.cpp)
void orbx_build_tables(const orbx_params &p, OrbxTables &t);
// returns ORBX_OK / ORBX_BAD_ASPECT / ORBX_UNSUPPORTED
orbx_status orbx_build_geometry(const orbx_params &p, const OrbxTables &t, int width, int height, OrbxGeom &g,
                                const char **why);
