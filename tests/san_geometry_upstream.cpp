// Sanitizer driver for csrc/orbx_geometry.cpp in ORBX_PYRAMID_UPSTREAM mode (tests/test_upstream_geometry.py builds it with
// g++ -fsanitize=address,undefined and runs it directly).  A level is the sw x sh view at (19, 19) of its padded buffer, so
//   * every resize tap reads the un-padded view of the previous level: slab index in [19, 19 + sw[l-1] - 1];
//   * every FAST cell lies inside the view;
//   * the narrow_taps verdict is the one a re-derivation from the tap table gives (k_pyr_resize_rows reads an aligned 12-byte
//     window around <= 8 consecutive source bytes per lane, inside the padded source row);
// and the values the Python model (tests/upstream_model.py) computes independently are printed, one line per level:
//   G w h level sw sh qt_w qt_h nini kp_cap ncols nrows wcell hcell ncells   then   C x0 y0 cw ch offx offy   per cell (view
//   coordinates), and   T w h kp_total   per size.  The error geometries print   E w h nlevels status.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_internal.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s (w=%d h=%d level=%d)\n", #c, w, h, l); ++fails; } } while (0)

static orbx_params params(int nl) {
    orbx_params p;
    std::memset(&p, 0, sizeof(p));
    p.nfeatures = 1000; p.scale_factor = 1.2f; p.nlevels = nl; p.ini_th_fast = 20; p.min_th_fast = 7;
    p.pyramid_mode = ORBX_PYRAMID_UPSTREAM; p.fp_mode = ORBX_FP_GCC_FMA; p.device = -2; p.max_batch = 1;
    return p;
}

static void one(int w, int h, bool expect_narrow) {
    const int nl = 8;
    const orbx_params p = params(nl);
    OrbxTables t;
    orbx_build_tables(p, t);
    OrbxGeom g;
    const char *why = "";
    int l = -1;
    const orbx_status st = orbx_build_geometry(p, t, w, h, g, &why);
    CHECK(st == ORBX_OK);
    if (st != ORBX_OK) return;
    CHECK(!g.l1_inplace);   // upstream handles take the eager level-0 copy
    for (l = 0; l < nl; ++l) {
        const OrbxLevelGeom &L = g.lv[l];
        CHECK(L.org == ORBX_EDGE && L.vw == L.sw && L.vh == L.sh && L.pw == L.sw + 38 && L.ph == L.sh + 38 && L.pitch >= L.pw);
        CHECK(L.off >= 0 && L.off + (long long)L.pitch * L.ph <= g.pyr_bytes);
        CHECK(L.qt_w == L.sw - 32 && L.qt_h == L.sh - 32 && L.qt_w > 0 && L.qt_h > 0 && L.nini >= 1);
        std::printf("G %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", w, h, l, L.sw, L.sh, L.qt_w, L.qt_h, L.nini, L.kp_cap, L.ncols,
                    L.nrows, L.wcell, L.hcell, L.cell_count);
        long long slots = 0;
        for (int c = L.cell_begin; c < L.cell_begin + L.cell_count; ++c) {
            const OrbxCell &C = g.cells[(size_t)c];
            // inside the view, in slab coordinates; the FAST region keeps 16 px to the view's edge
            CHECK(C.level == l && C.x0 >= 19 + 16 && C.y0 >= 19 + 16 && C.x0 + C.cw <= 19 + L.sw - 16 && C.y0 + C.ch <= 19 + L.sh - 16);
            CHECK(C.cw >= 7 && C.ch >= 7 && C.slot_begin == slots && C.slot_cap >= 1);
            slots += C.slot_cap;
            std::printf("C %d %d %d %d %d %d\n", C.x0 - 19, C.y0 - 19, C.cw, C.ch, C.offx, C.offy);
        }
        CHECK(slots <= L.cand_cap);
        if (l == 0) continue;
        const OrbxLevelGeom &S = g.lv[l - 1];
        for (int x = 0; x < L.pw; ++x) {
            const OrbxTap &T = g.taps[(size_t)L.tapx_begin + x];
            CHECK(T.s0 >= 19 && T.s1 <= 19 + S.sw - 1 && T.s0 <= T.s1 && T.a0 + T.a1 == 2048);
        }
        for (int y = 0; y < L.ph; ++y) {
            const OrbxTap &T = g.taps[(size_t)L.tapy_begin + y];
            CHECK(T.s0 >= 19 && T.s1 <= 19 + S.sh - 1 && T.s0 <= T.s1 && T.a0 + T.a1 == 2048);
        }
        // the border of the destination is the reflection of its centre: padded column P and its mirror image share one tap
        for (int P = 0; P < 19; ++P) {
            const OrbxTap &a = g.taps[(size_t)L.tapx_begin + P], &b = g.taps[(size_t)L.tapx_begin + 19 + (19 - P)];
            CHECK(a.s0 == b.s0 && a.s1 == b.s1 && a.a0 == b.a0 && a.a1 == b.a1);
        }
        bool narrow = true;
        for (int X = 0; X < L.pw; X += 4) {
            int lo = 0x7fff, hi = 0;
            for (int i = 0; i < 4; ++i) {
                const OrbxTap &T = g.taps[(size_t)L.tapx_begin + std::min(X + i, L.pw - 1)];
                lo = std::min<int>(lo, T.s0); hi = std::max<int>(hi, T.s0);
                if (T.s1 != T.s0 + 1 && T.a1 != 0) narrow = false;
            }
            if (hi + 2 - lo > 8) narrow = false;
            // the aligned 12-byte window of k_pyr_resize_rows stays inside the padded source row
            CHECK((lo & ~3) + 12 <= S.pitch && (lo & ~3) >= 0);
        }
        CHECK(L.narrow_taps == narrow);
        CHECK(L.narrow_taps == expect_narrow);
    }
    l = -1;
    int sum = 0;
    for (int k = 0; k < nl; ++k) sum += g.lv[k].kp_cap;
    CHECK(g.kp_total == sum);
    std::printf("T %d %d %d\n", w, h, g.kp_total);
    for (const OrbxFastGroup &G : g.fast_groups) {
        CHECK(G.ncell == 1 || G.ncell == 2);
        const OrbxCell &a = g.cells[(size_t)G.cell0], &b = g.cells[(size_t)G.cell0 + G.ncell - 1];
        CHECK(a.level == b.level && a.y0 == b.y0 && b.x0 + b.cw - a.x0 - 6 <= 64 + ORBX_FAST_XCOLS);
    }
}

static void refused(int w, int h, int nl) {
    const orbx_params p = params(nl);
    OrbxTables t;
    orbx_build_tables(p, t);
    OrbxGeom g;
    const char *why = "";
    const orbx_status st = orbx_build_geometry(p, t, w, h, g, &why);
    std::printf("E %d %d %d %d %s\n", w, h, nl, (int)st, why);
}

int main() {
    one(640, 480, true); one(752, 480, true); one(1241, 376, true); one(300, 200, true); one(160, 120, true);
    refused(200, 96, 8);    // level 6 is 67 x 32: FAST region 35 x 0
    refused(97, 131, 8);    // nIni == 0 at level 4
    refused(97, 131, 4);    // fine with 4 levels
    std::printf("upstream geometry sanitizer run: %d failures\n", fails);
    return fails != 0;
}
