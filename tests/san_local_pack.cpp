// san_local_pack.cpp -- stand-alone driver of csrc/orbx_track_pack.cpp for AddressSanitizer + UndefinedBehaviorSanitizer: the
// part behind orbx_search_local_points_batch_device (validation, layout, packing of the shared pool and the problems) and the
// PredictScale threshold table (tests/test_local_points_cpu.py builds and runs it as a child process).  Every view is an exactly
// sized heap block, so that a read past an array is a report; the staging block is exactly plan.in_bytes long and is checked
// against the inputs after packing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_track.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static std::mt19937 rng(11);
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); }

struct Pool {
    std::vector<float> pos, nrm, dmin, dmax; std::vector<uint8_t> desc; std::vector<int32_t> obs;
    explicit Pool(int n) : pos((size_t)n * 3), nrm((size_t)n * 3), dmin(n), dmax(n), desc((size_t)n * 32), obs(n) {
        for (auto &v : pos) v = (float)rnd(-50, 50) * 0.1f;
        for (auto &v : nrm) v = (float)rnd(-10, 10) * 0.1f;
        for (int i = 0; i < n; ++i) { dmin[i] = 0.5f + (float)i; dmax[i] = 4.0f + (float)i; obs[i] = rnd(0, 3); }
        for (auto &b : desc) b = (uint8_t)rnd(0, 255);
    }
    orbx_local_map_view view() const {
        orbx_local_map_view v; memset(&v, 0, sizeof(v));
        v.n = (int32_t)obs.size();
        if (v.n) { v.world_pos = pos.data(); v.normal = nrm.data(); v.min_distance = dmin.data(); v.max_distance = dmax.data();
                   v.desc = desc.data(); v.observations = obs.data(); }
        return v;
    }
};
struct Problem {
    std::vector<int32_t> index, fobs; std::vector<uint8_t> skip;
    bool whole = false, with_skip = true, with_fobs = true;
    int frame = 0; float th = 3.f;
    orbx_track_local_problem view(int npool) const {
        orbx_track_local_problem p; memset(&p, 0, sizeof(p));
        p.frame = frame; p.th = th; p.viewing_cos_limit = 0.5f;
        for (int i = 0; i < 16; ++i) p.Tcw[i] = (float)(i + 1) + 0.25f * (float)frame;
        for (int i = 0; i < 3; ++i) p.Ow[i] = -(float)(i + 1);
        p.npoints = whole ? npool : (int32_t)index.size();
        p.point_index = whole || index.empty() ? nullptr : index.data();
        p.skip = with_skip && !skip.empty() ? skip.data() : nullptr;
        p.frame_observations = with_fobs && !fobs.empty() ? fobs.data() : nullptr;
        return p;
    }
};
static Problem make_problem(int npool, int cap, int nframes) {
    Problem P;
    P.frame = rnd(0, nframes - 1); P.th = rnd(0, 1) ? 1.f : 3.f;
    P.whole = npool > 0 && rnd(0, 3) == 0;
    const int n = P.whole ? npool : npool ? rnd(0, 2 * npool) : 0;
    P.index.resize(P.whole ? 0 : n);
    for (auto &i : P.index) i = rnd(0, npool - 1);
    P.with_skip = rnd(0, 2) != 0; P.with_fobs = rnd(0, 2) != 0;
    P.skip.resize(n);
    for (auto &s : P.skip) s = (uint8_t)(rnd(0, 9) == 0 ? rnd(1, 255) : 0);
    P.fobs.resize(cap);
    for (auto &o : P.fobs) o = rnd(-1, 2);
    return P;
}

static orbx_status plan_of(const std::vector<orbx_track_local_problem> &v, const orbx_local_map_view *map, int nframes, int cap,
                           OrbxLocalPlan &plan, const char **why, bool dev_ok = true, int n = -2) {
    const OrbxTrackBatchArgs a = {nframes, cap, 8, dev_ok};
    *why = "";
    return orbx_track_local_plan(n == -2 ? (int)v.size() : n, v.empty() ? nullptr : v.data(), map, a, plan, why);
}

static void check_packed(const Pool &pool, const std::vector<Problem> &probs, int nframes, int cap) {
    const orbx_local_map_view mv = pool.view();
    const int npool = mv.n;
    std::vector<orbx_track_local_problem> v;
    for (const Problem &P : probs) v.push_back(P.view(npool));
    OrbxLocalPlan plan; const char *why;
    CHECK(plan_of(v, &mv, nframes, cap, plan, &why) == ORBX_OK);
    CHECK(plan.in_bytes % 256 == 0 && plan.dev_bytes >= plan.in_bytes && plan.o_q == plan.in_bytes);
    CHECK(plan.o_pdesc % 32 == 0 && plan.o_desc % 32 == 0 && plan.o_cand % 16 == 0);
    std::vector<uint8_t> block(plan.in_bytes, 0xcd);
    orbx_track_local_pack((int)v.size(), v.data(), &mv, plan, cap, block.data());
    const DTrackProb *dp = (const DTrackProb *)(block.data() + plan.o_prob);
    const DTrackLocal *dl = (const DTrackLocal *)(block.data() + plan.o_local);
    const DTrackPoolPt *pp = (const DTrackPoolPt *)(block.data() + plan.o_pool);
    const int32_t *di = (const int32_t *)(block.data() + plan.o_index);
    const uint8_t *dk = block.data() + plan.o_skip;
    const uint32_t *ds = (const uint32_t *)(block.data() + plan.o_seed);
    for (int i = 0; i < npool; ++i) {
        CHECK(pp[i].P[2] == pool.pos[3 * (size_t)i + 2] && pp[i].Pn[0] == pool.nrm[3 * (size_t)i] && pp[i].dmin == pool.dmin[i] &&
              pp[i].dmax == pool.dmax[i] && pp[i].obs == pool.obs[i]);
    }
    CHECK(npool == 0 || memcmp(block.data() + plan.o_pdesc, pool.desc.data(), (size_t)npool * 32) == 0);
    size_t base = 0; int maxp = 0;
    for (size_t k = 0; k < probs.size(); ++k) {
        const orbx_track_local_problem &P = v[k];
        CHECK(dp[k].frame == P.frame && dp[k].q_begin == (int32_t)base && dp[k].nq == P.npoints && dp[k].dir == 0);
        CHECK(dp[k].Rcw[5] == P.Tcw[6] && dp[k].tcw[1] == P.Tcw[7] && dl[k].Ow[2] == P.Ow[2] && dl[k].th == P.th && dl[k].cos_limit == 0.5f);
        for (int i = 0; i < P.npoints; ++i) {
            CHECK(di[base + i] == (P.point_index ? P.point_index[i] : i) && di[base + i] >= 0 && di[base + i] < npool);
            CHECK(dk[base + i] == (P.skip && P.skip[i] ? 1 : 0));
        }
        for (int i = 0; i < cap; ++i)
            CHECK(((ds[k * plan.seed_words + (i >> 5)] >> (i & 31)) & 1u) == (P.frame_observations && P.frame_observations[i] > 0 ? 1u : 0u));
        base += (size_t)P.npoints;
        if (P.npoints > maxp) maxp = P.npoints;
    }
    CHECK(base == plan.nq && maxp == plan.max_points);
}

static void check_table(float scale_factor, int nlevels) {
    float thr[ORBX_PS_LEVELS];
    orbx_predict_scale_build(scale_factor, nlevels, thr);
    const float lsf = logf(scale_factor);
    CHECK(thr[0] == 0.f);
    for (int k = 1; k < ORBX_PS_LEVELS; ++k) {
        if (k >= nlevels || std::isinf(thr[k])) { CHECK(std::isinf(thr[k]) && thr[k] > 0); continue; }
        // (a factor next to 1 makes the expression skip levels: two thresholds may then coincide)
        CHECK(thr[k] >= thr[k - 1] && (int)ceilf(logf(thr[k]) / lsf) >= k);
        const float before = std::nextafter(thr[k], 0.f);
        CHECK(before > 0.f && (int)ceilf(logf(before) / lsf) < k);
        CHECK(orbx_predict_scale_level(thr, nlevels, thr[k]) >= k && orbx_predict_scale_level(thr, nlevels, before) <= k - 1);
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(orbx_predict_scale_level(thr, nlevels, nan) == 0 && orbx_predict_scale_level(thr, nlevels, -1.f) == 0 &&
          orbx_predict_scale_level(thr, nlevels, 0.f) == 0 && orbx_predict_scale_level(thr, nlevels, -inf) == 0);
    CHECK(orbx_predict_scale_level(thr, nlevels, inf) == nlevels - 1);
    for (int t = 0; t < 20000; ++t) {   // the levels of the expression itself
        const float ratio = std::ldexp(1.f + (float)rnd(0, 1 << 23) / (float)(1 << 23), rnd(-4, 7));
        int want = (int)ceilf(logf(ratio) / lsf);
        want = want < 0 ? 0 : want >= nlevels ? nlevels - 1 : want;
        CHECK(orbx_predict_scale_level(thr, nlevels, ratio) == want);
    }
}

int main() {
    const int nframes = 3, cap = 70;   // cap: two seed words and a bit
    const float factors[] = {1.2f, 2.0f, 1.1f, 1.0000001f, 1.0e10f};
    for (float f : factors)
        for (int nl : {1, 2, 8, 16}) check_table(f, nl);

    OrbxLocalPlan plan; const char *why;
    const Pool pool(9);
    const orbx_local_map_view mv = pool.view();
    // nothing to do; empty pools and problems
    { std::vector<orbx_track_local_problem> none;
      CHECK(plan_of(none, nullptr, 0, cap, plan, &why) == ORBX_OK && plan.nq == 0);
      CHECK(plan_of(none, &mv, nframes, cap, plan, &why) == ORBX_OK && plan.npool == 9);
      check_packed(Pool(0), {Problem(), Problem()}, nframes, cap);
      Problem e; e.fobs.resize(cap);
      check_packed(pool, {e, e}, nframes, cap); }
    // every rejection
    { Problem g = make_problem(9, cap, nframes);
      g.whole = false; g.index = {0, 8, 3, 3};  g.skip.assign(4, 0);
      std::vector<orbx_track_local_problem> v = {g.view(9), g.view(9)};
      CHECK(plan_of(v, &mv, nframes, cap, plan, &why) == ORBX_OK && plan.nq == 8 && plan.max_points == 4);
      CHECK(plan_of(v, &mv, nframes, cap, plan, &why, true, -1) == ORBX_BAD_ARGUMENT && strstr(why, "nproblems"));
      CHECK(plan_of(v, &mv, nframes, 0, plan, &why) == ORBX_BAD_ARGUMENT && strstr(why, "cap"));
      CHECK(plan_of(v, &mv, nframes, 65536, plan, &why) == ORBX_UNSUPPORTED && strstr(why, "65535"));
      CHECK(plan_of(v, &mv, 0, cap, plan, &why) == ORBX_BAD_ARGUMENT && strstr(why, "nframes"));
      CHECK(plan_of(v, &mv, nframes, cap, plan, &why, false) == ORBX_BAD_ARGUMENT && strstr(why, "device buffer"));
      CHECK(plan_of(v, nullptr, nframes, cap, plan, &why) == ORBX_BAD_ARGUMENT && strstr(why, "null local map"));
      { const OrbxTrackBatchArgs a = {nframes, cap, 8, true};
        CHECK(orbx_track_local_plan(2, nullptr, &mv, a, plan, &why) == ORBX_BAD_ARGUMENT && strstr(why, "problem array")); }
      v[1].frame = nframes;
      CHECK(plan_of(v, &mv, nframes, cap, plan, &why) == ORBX_BAD_ARGUMENT && strstr(why, "frame outside"));
      v[1].frame = -1;
      CHECK(plan_of(v, &mv, nframes, cap, plan, &why) == ORBX_BAD_ARGUMENT && strstr(why, "frame outside"));
      v[1].frame = 0; v[1].npoints = -1;
      CHECK(plan_of(v, &mv, nframes, cap, plan, &why) == ORBX_BAD_ARGUMENT && strstr(why, "npoints"));
      v[1].npoints = 4;
      for (int bad : {9, -1, 0x7fffffff}) {
          Problem b = g; b.index[3] = bad;
          v[1] = b.view(9);
          CHECK(plan_of(v, &mv, nframes, cap, plan, &why) == ORBX_BAD_ARGUMENT && strstr(why, "point_index outside"));
      }
      v[1] = g.view(9); v[1].point_index = nullptr;                 // NULL: the whole pool, so npoints must be its n
      CHECK(plan_of(v, &mv, nframes, cap, plan, &why) == ORBX_BAD_ARGUMENT && strstr(why, "point_index is NULL"));
      v[1].npoints = 9;
      CHECK(plan_of(v, &mv, nframes, cap, plan, &why) == ORBX_OK && plan.nq == 13 && plan.max_points == 9);
      v[1] = g.view(9);
      for (int f = 0; f < 6; ++f) {
          orbx_local_map_view m2 = mv;
          switch (f) {
          case 0: m2.world_pos = nullptr; break;
          case 1: m2.normal = nullptr; break;
          case 2: m2.min_distance = nullptr; break;
          case 3: m2.max_distance = nullptr; break;
          case 4: m2.desc = nullptr; break;
          default: m2.observations = nullptr; break;
          }
          CHECK(plan_of(v, &m2, nframes, cap, plan, &why) == ORBX_BAD_ARGUMENT && strstr(why, "null field"));
      }
      orbx_local_map_view m3 = mv; m3.n = -1;
      CHECK(plan_of(v, &m3, nframes, cap, plan, &why) == ORBX_BAD_ARGUMENT && strstr(why, "map.n"));
      const Pool none(0); const orbx_local_map_view m0 = none.view();   // an index into an empty pool
      CHECK(plan_of(v, &m0, nframes, cap, plan, &why) == ORBX_BAD_ARGUMENT && strstr(why, "point_index outside")); }
    // random calls, packed and read back
    for (int t = 0; t < 200; ++t) {
        const int npool = t % 7 == 0 ? 1 : rnd(1, 60), c = t % 5 == 0 ? 32 : t % 5 == 1 ? 1 : cap;
        const Pool P(npool);
        std::vector<Problem> probs;
        for (int k = rnd(1, 6); k > 0; --k) probs.push_back(make_problem(npool, c, nframes));
        check_packed(P, probs, nframes, c);
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
