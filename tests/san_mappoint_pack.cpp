// san_mappoint_pack.cpp -- stand-alone driver of csrc/orbx_mappoint.cpp (the HIP-free validation, size-class plan, packing and
// scatter of the batched MapPoint refresh) for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_mappoint_batch_cpu.py
// builds and runs it).  Every caller array is an exactly sized heap block, so that a read or write past one is a report; the
// staging block is exactly plan.in_bytes long and is read back, the download block exactly plan.out_bytes.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_mappoint.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static std::mt19937 rng(11);
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); }

static std::vector<int32_t> begins(const std::vector<int> &n) {
    std::vector<int32_t> b(n.size() + 1, 0);
    for (size_t i = 0; i < n.size(); ++i) b[i + 1] = b[i] + n[i];
    return b;
}

// plans, packs and scatters one ragged batch in both forms; checks the order list, the row payload and the untouched rows
static void run_distinct(const std::vector<int> &n) {
    const int P = (int)n.size();
    const std::vector<int32_t> b = begins(n);
    const size_t rows = (size_t)b[P];
    std::vector<uint8_t> desc(rows * 32);
    for (auto &v : desc) v = (uint8_t)rnd(0, 255);
    std::vector<int64_t> obs_row(rows);
    const int64_t pool_rows = 5000;
    for (auto &v : obs_row) v = rnd(0, (int)pool_rows - 1);
    alignas(16) static uint8_t pool_tag[16];
    for (int form = 0; form < 2; ++form) {
        OrbxMpPlan plan;
        const char *why = "";
        std::vector<int32_t> idx((size_t)P, 7), med((size_t)P, 7);
        std::vector<uint8_t> out((size_t)P * 32, 0xA5);
        const orbx_status st = orbx_mp_distinct_plan(P, b.data(), rows ? desc.data() : nullptr, form == 1, pool_tag, pool_rows,
                                                     rows ? obs_row.data() : nullptr, idx.data(), plan, &why);
        CHECK(st == ORBX_OK);
        if (st != ORBX_OK) { printf("  %s\n", why); continue; }
        int small = 0, wide = 0;
        for (int v : n) { small += v >= 1 && v <= ORBX_MP_GROUP; wide += v > ORBX_MP_GROUP; }
        CHECK(plan.n_small == small && plan.n_wide == wide && plan.nrows == rows && plan.npoints == P);
        CHECK(plan.in_bytes % 256 == 0 && plan.o_idx == plan.in_bytes && plan.out_bytes == plan.dev_bytes - plan.o_idx);
        std::vector<uint8_t> block(plan.in_bytes, 0xEE);
        orbx_mp_distinct_pack(b.data(), rows ? desc.data() : nullptr, form == 1 ? obs_row.data() : nullptr, plan, block.data());
        CHECK(memcmp(block.data() + plan.o_begin, b.data(), ((size_t)P + 1) * 4) == 0);
        const int32_t *order = (const int32_t *)(block.data() + plan.o_order);
        int prev = -1;
        for (int k = 0; k < small + wide; ++k) {
            if (k == small) prev = -1;
            const int p = order[k];
            CHECK(p > prev && p < P);
            if (p < 0 || p >= P) break;
            CHECK(k < small ? (n[p] >= 1 && n[p] <= ORBX_MP_GROUP) : n[p] > ORBX_MP_GROUP);
            prev = p;
        }
        if (rows) {
            if (form == 1) CHECK(memcmp(block.data() + plan.o_rows, obs_row.data(), rows * 8) == 0);
            else CHECK(memcmp(block.data() + plan.o_rows, desc.data(), rows * 32) == 0);
        }
        // what the device would send back: idx = p, med = 2 p, desc rows = p
        std::vector<uint8_t> down(plan.out_bytes, 0);
        for (int p = 0; p < P; ++p) {
            ((int32_t *)down.data())[p] = p;
            ((int32_t *)(down.data() + (plan.o_med - plan.o_idx)))[p] = 2 * p;
            memset(down.data() + (plan.o_desc - plan.o_idx) + (size_t)p * 32, p & 0x7f, 32);
        }
        orbx_mp_distinct_unpack(b.data(), plan, down.data(), idx.data(), form ? nullptr : med.data(), form ? nullptr : out.data());
        for (int p = 0; p < P; ++p) {
            CHECK(idx[p] == (n[p] ? p : -1));
            if (form == 0) {
                CHECK(med[p] == (n[p] ? 2 * p : -1));
                for (int k = 0; k < 32; ++k) CHECK(out[(size_t)p * 32 + k] == (n[p] ? (uint8_t)(p & 0x7f) : 0xA5));
            }
        }
    }
}

static void run_normal(const std::vector<int> &n, int nlevels) {
    const int P = (int)n.size();
    const std::vector<int32_t> b = begins(n);
    const size_t rows = (size_t)b[P];
    std::vector<float> pos((size_t)P * 3), refc((size_t)P * 3), centers(rows * 3), scale((size_t)nlevels, 1.f);
    for (int l = 1; l < nlevels; ++l) scale[l] = scale[l - 1] * 1.2f;
    for (auto &v : pos) v = (float)rnd(-500, 500) * 0.01f;
    for (auto &v : refc) v = (float)rnd(-500, 500) * 0.01f;
    for (auto &v : centers) v = (float)rnd(-500, 500) * 0.01f;
    std::vector<int32_t> level((size_t)P);
    for (int p = 0; p < P; ++p) level[p] = n[p] ? rnd(0, nlevels - 1) : 1000 + p;   // not looked at on a point without rows
    std::vector<float> normal((size_t)P * 3, -7.f), dmin((size_t)P, -7.f), dmax((size_t)P, -7.f);
    OrbxMpNormalPlan plan;
    const char *why = "";
    const orbx_status st = orbx_mp_normal_plan(P, b.data(), pos.data(), rows ? centers.data() : nullptr, refc.data(), level.data(),
                                               nlevels, normal.data(), dmin.data(), dmax.data(), plan, &why);
    CHECK(st == ORBX_OK);
    if (st != ORBX_OK) { printf("  %s\n", why); return; }
    std::vector<uint8_t> block(plan.in_bytes, 0xEE);
    orbx_mp_normal_pack(b.data(), pos.data(), rows ? centers.data() : nullptr, refc.data(), level.data(), scale.data(), plan,
                        block.data());
    const DMpPoint *pt = (const DMpPoint *)(block.data() + plan.o_points);
    for (int p = 0; p < P; ++p) {
        CHECK(memcmp(pt[p].pos, &pos[3 * (size_t)p], 12) == 0 && memcmp(pt[p].ref, &refc[3 * (size_t)p], 12) == 0);
        CHECK(pt[p].level_scale == (n[p] ? scale[level[p]] : 0.f));
    }
    if (rows) CHECK(memcmp(block.data() + plan.o_centers, centers.data(), rows * 12) == 0);
    std::vector<uint8_t> down(plan.out_bytes, 0);
    for (int p = 0; p < P; ++p)
        for (int c = 0; c < 5; ++c) ((float *)down.data())[5 * (size_t)p + c] = (float)(10 * p + c);
    orbx_mp_normal_unpack(b.data(), plan, down.data(), normal.data(), dmin.data(), dmax.data());
    for (int p = 0; p < P; ++p) {
        for (int c = 0; c < 3; ++c) CHECK(normal[3 * (size_t)p + c] == (n[p] ? (float)(10 * p + c) : -7.f));
        CHECK(dmin[p] == (n[p] ? (float)(10 * p + 3) : -7.f) && dmax[p] == (n[p] ? (float)(10 * p + 4) : -7.f));
    }
}

static void rejections() {
    OrbxMpPlan plan; OrbxMpNormalPlan np;
    const char *why = "";
    const int32_t good[4] = {0, 2, 2, 5}, dec[4] = {0, 3, 2, 5}, first[4] = {1, 2, 2, 5};
    std::vector<uint8_t> desc(5 * 32, 1);
    std::vector<int64_t> rows = {0, 1, 2, 3, 9};
    alignas(16) static uint8_t pool[32];
    int32_t idx[3];
    const int B = ORBX_BAD_ARGUMENT;
    CHECK(orbx_mp_distinct_plan(-1, good, desc.data(), false, nullptr, 0, nullptr, idx, plan, &why) == B);
    CHECK(orbx_mp_distinct_plan(0, nullptr, nullptr, false, nullptr, 0, nullptr, nullptr, plan, &why) == ORBX_OK);
    CHECK(orbx_mp_distinct_plan(3, nullptr, desc.data(), false, nullptr, 0, nullptr, idx, plan, &why) == B);
    CHECK(orbx_mp_distinct_plan(3, dec, desc.data(), false, nullptr, 0, nullptr, idx, plan, &why) == B);
    CHECK(orbx_mp_distinct_plan(3, first, desc.data(), false, nullptr, 0, nullptr, idx, plan, &why) == B);
    CHECK(orbx_mp_distinct_plan(3, good, nullptr, false, nullptr, 0, nullptr, idx, plan, &why) == B);
    CHECK(orbx_mp_distinct_plan(3, good, desc.data(), false, nullptr, 0, nullptr, nullptr, plan, &why) == B);
    CHECK(orbx_mp_distinct_plan(3, good, desc.data(), false, nullptr, 0, nullptr, idx, plan, &why) == ORBX_OK);
    CHECK(orbx_mp_distinct_plan(3, good, nullptr, true, pool, 10, rows.data(), idx, plan, &why) == ORBX_OK);
    CHECK(orbx_mp_distinct_plan(3, good, nullptr, true, pool, 9, rows.data(), idx, plan, &why) == B);      // row 9 of 9
    CHECK(orbx_mp_distinct_plan(3, good, nullptr, true, pool, -1, rows.data(), idx, plan, &why) == B);
    CHECK(orbx_mp_distinct_plan(3, good, nullptr, true, pool + 4, 10, rows.data(), idx, plan, &why) == B);  // alignment
    CHECK(orbx_mp_distinct_plan(3, good, nullptr, true, nullptr, 10, rows.data(), idx, plan, &why) == B);
    CHECK(orbx_mp_distinct_plan(3, good, nullptr, true, pool, 10, nullptr, idx, plan, &why) == B);
    rows[2] = -1;
    CHECK(orbx_mp_distinct_plan(3, good, nullptr, true, pool, 10, rows.data(), idx, plan, &why) == B);
    std::vector<float> f3(9, 0.f), c(15, 0.f), o1(3, 0.f);
    int32_t lvl[3] = {0, 99, 7};                                     // point 1 has no rows: its level is not looked at
    CHECK(orbx_mp_normal_plan(3, good, f3.data(), c.data(), f3.data(), lvl, 8, f3.data(), o1.data(), o1.data(), np, &why) == ORBX_OK);
    lvl[2] = 8;
    CHECK(orbx_mp_normal_plan(3, good, f3.data(), c.data(), f3.data(), lvl, 8, f3.data(), o1.data(), o1.data(), np, &why) == B);
    lvl[2] = -1;
    CHECK(orbx_mp_normal_plan(3, good, f3.data(), c.data(), f3.data(), lvl, 8, f3.data(), o1.data(), o1.data(), np, &why) == B);
    lvl[2] = 3;
    CHECK(orbx_mp_normal_plan(-2, good, f3.data(), c.data(), f3.data(), lvl, 8, f3.data(), o1.data(), o1.data(), np, &why) == B);
    CHECK(orbx_mp_normal_plan(0, nullptr, nullptr, nullptr, nullptr, nullptr, 8, nullptr, nullptr, nullptr, np, &why) == ORBX_OK);
    CHECK(orbx_mp_normal_plan(3, dec, f3.data(), c.data(), f3.data(), lvl, 8, f3.data(), o1.data(), o1.data(), np, &why) == B);
    CHECK(orbx_mp_normal_plan(3, good, nullptr, c.data(), f3.data(), lvl, 8, f3.data(), o1.data(), o1.data(), np, &why) == B);
    CHECK(orbx_mp_normal_plan(3, good, f3.data(), nullptr, f3.data(), lvl, 8, f3.data(), o1.data(), o1.data(), np, &why) == B);
    CHECK(orbx_mp_normal_plan(3, good, f3.data(), c.data(), nullptr, lvl, 8, f3.data(), o1.data(), o1.data(), np, &why) == B);
    CHECK(orbx_mp_normal_plan(3, good, f3.data(), c.data(), f3.data(), nullptr, 8, f3.data(), o1.data(), o1.data(), np, &why) == B);
    CHECK(orbx_mp_normal_plan(3, good, f3.data(), c.data(), f3.data(), lvl, 8, nullptr, o1.data(), o1.data(), np, &why) == B);
    CHECK(orbx_mp_normal_plan(3, good, f3.data(), c.data(), f3.data(), lvl, 8, f3.data(), nullptr, o1.data(), np, &why) == B);
    CHECK(orbx_mp_normal_plan(3, good, f3.data(), c.data(), f3.data(), lvl, 8, f3.data(), o1.data(), nullptr, np, &why) == B);
}

int main() {
    rejections();
    const int G = ORBX_MP_GROUP, W = ORBX_MP_LDS_ROWS;
    const std::vector<std::vector<int> > cases = {
        {0}, {0, 0, 0}, {1}, {300},
        {0, 3, 0, 5, 0},                                             // no rows at the front, in the middle, at the end
        {0, 0, 2, 17, 0, 0, 64, 1, 0},
        {1, G - 1, G, G + 1, 63, 64, 65, W - 1, W, W + 1},           // every size-class boundary
        {G + 1, 1, G, 2, 300, 0, 3},
    };
    for (const auto &n : cases) { run_distinct(n); run_normal(n, 8); }
    for (int it = 0; it < 60; ++it) {
        std::vector<int> n((size_t)rnd(1, 80));
        for (auto &v : n) v = rnd(0, 9) == 0 ? 0 : rnd(0, 4) == 0 ? rnd(1, 90) : rnd(1, 9);
        run_distinct(n);
        run_normal(n, rnd(1, 12));
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
