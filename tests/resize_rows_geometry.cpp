// resize_rows_geometry.cpp -- what tests/test_resize_rows_gpu.py needs to know about a geometry without a GPU, from
// csrc/orbx_geometry.cpp itself (built together with it by that test).  Host only.
//
// usage: resize_rows_geometry W H scale_factor nlevels upstream [W H scale_factor nlevels upstream ...]
// For each geometry one line
//   geo W H sf nl up status S l1_inplace I l1_tail_bx T taps N hash X
// where X is a 64-bit FNV-1a hash over the tap records a ROW of a level names -- every level's pw horizontal and ph vertical
// records (and the raw-coordinate level-1 table's), in level order, each as (s0, s1, a0, a1) -- but not over the record the
// row walk may read beyond a level's last row; then one line `level l pw ph` per level.
// Checked here (a `FAIL` line and exit status 1): the record beyond the last row of every vertical table exists, repeats the
// last row's record (so its source rows are rows of the source level), and lies in no level's horizontal or vertical range.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <utility>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_internal.h"

static long g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { ++g_fail; printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t fnv(uint64_t h, const OrbxTap &t) {
    const int16_t v[4] = {t.s0, t.s1, t.a0, t.a1};
    for (int i = 0; i < 4; ++i)
        for (int b = 0; b < 2; ++b) { h ^= (uint64_t)(((uint16_t)v[i] >> (8 * b)) & 0xff); h *= 1099511628211ull; }
    return h;
}

int main(int argc, char **argv) {
    for (int a = 1; a + 4 < argc; a += 5) {
        const int W = atoi(argv[a]), H = atoi(argv[a + 1]), nl = atoi(argv[a + 3]), up = atoi(argv[a + 4]);
        orbx_params p;
        memset(&p, 0, sizeof(p));
        p.nfeatures = 1000; p.scale_factor = (float)atof(argv[a + 2]); p.nlevels = nl; p.ini_th_fast = 20; p.min_th_fast = 7; p.max_batch = 1;
        p.pyramid_mode = up ? ORBX_PYRAMID_UPSTREAM : ORBX_PYRAMID_FORK_PADDED;
        OrbxTables t;
        OrbxGeom g;
        const char *why = "";
        orbx_build_tables(p, t);
        const orbx_status st = orbx_build_geometry(p, t, W, H, g, &why);
        uint64_t h = 14695981039346656037ull;
        std::vector<std::pair<size_t, size_t>> rows_of;   // [begin, end) ranges of records that belong to a row or column
        std::vector<size_t> pads;
        if (st == ORBX_OK) {
            for (int l = 1; l < nl; ++l) {
                const OrbxLevelGeom &L = g.lv[l];
                rows_of.push_back({(size_t)L.tapx_begin, (size_t)L.tapx_begin + L.pw});
                rows_of.push_back({(size_t)L.tapy_begin, (size_t)L.tapy_begin + L.ph});
                pads.push_back((size_t)L.tapy_begin + L.ph);
            }
            if (g.l1_tap_begin > 0) {
                const OrbxLevelGeom &L = g.lv[1];
                rows_of.push_back({(size_t)g.l1_tap_begin, (size_t)g.l1_tap_begin + L.pw + L.ph});
                pads.push_back((size_t)g.l1_tap_begin + L.pw + L.ph);
            }
            for (const auto &r : rows_of) {
                CHECK(r.second <= g.taps.size(), "range [%zu, %zu) of %zu records", r.first, r.second, g.taps.size());
                for (size_t i = r.first; i < r.second && i < g.taps.size(); ++i) h = fnv(h, g.taps[i]);
            }
            for (size_t q : pads) {
                CHECK(q < g.taps.size(), "no record beyond the last row at %zu of %zu", q, g.taps.size());
                if (q >= g.taps.size()) continue;
                CHECK(memcmp(&g.taps[q], &g.taps[q - 1], sizeof(OrbxTap)) == 0, "record %zu does not repeat the last row's", q);
                for (const auto &r : rows_of) CHECK(q < r.first || q >= r.second, "record %zu beyond a last row is a tap of [%zu, %zu)", q, r.first, r.second);
            }
        }
        printf("geo %d %d %s %d %d status %d l1_inplace %d l1_tail_bx %d taps %zu hash %016llx\n", W, H, argv[a + 2], nl, up, (int)st,
               (int)g.l1_inplace, g.l1_tail_bx, g.taps.size(), (unsigned long long)h);
        if (st != ORBX_OK) { printf("FAIL geometry: %s\n", why); ++g_fail; continue; }
        for (int l = 0; l < nl; ++l) printf("level %d %d %d\n", l, g.lv[l].pw, g.lv[l].ph);
    }
    return g_fail ? 1 : 0;
}
