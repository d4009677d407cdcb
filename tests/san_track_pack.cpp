// san_track_pack.cpp -- stand-alone driver of csrc/orbx_track_pack.cpp (the HIP-free validation + packing unit of the batched
// tracking matchers) for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_track_batch_cpu.py builds and runs it).
// Every view is an exactly sized heap block, so that a read past an array is a report; the staging block is exactly
// plan.in_bytes long and is read back in full after packing.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_track.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

struct LastFrame {
    std::vector<orbx_keypoint> keys; std::vector<uint8_t> has, desc; std::vector<float> xw; std::vector<int32_t> obs;
    orbx_last_frame_view view() const {
        orbx_last_frame_view v; memset(&v, 0, sizeof(v));
        v.n = (int32_t)keys.size();
        v.keys_un = keys.empty() ? nullptr : keys.data(); v.has_map_point = has.empty() ? nullptr : has.data();
        v.world_pos = xw.empty() ? nullptr : xw.data(); v.mp_desc = desc.empty() ? nullptr : desc.data();
        v.observations = obs.empty() ? nullptr : obs.data();
        for (int i = 0; i < 4; ++i) v.Tcw[5 * i] = 1.f;
        return v;
    }
};
struct Points {
    std::vector<uint8_t> in_view, desc; std::vector<float> proj, cosv; std::vector<int32_t> level, obs;
    orbx_mappoint_view view() const {
        orbx_mappoint_view v; memset(&v, 0, sizeof(v));
        v.n = (int32_t)in_view.size();
        v.in_view = in_view.empty() ? nullptr : in_view.data(); v.proj = proj.empty() ? nullptr : proj.data();
        v.level = level.empty() ? nullptr : level.data(); v.view_cos = cosv.empty() ? nullptr : cosv.data();
        v.desc = desc.empty() ? nullptr : desc.data(); v.observations = obs.empty() ? nullptr : obs.data();
        return v;
    }
};

static std::mt19937 rng(7);
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); }

static LastFrame make_last(int n, int nlevels) {
    LastFrame L;
    L.keys.resize(n); L.has.resize(n); L.desc.resize((size_t)n * 32); L.xw.resize((size_t)n * 3); L.obs.resize(n);
    for (int i = 0; i < n; ++i) {
        memset(&L.keys[i], 0, sizeof(orbx_keypoint));
        L.keys[i].octave = rnd(0, nlevels - 1); L.keys[i].angle = (float)rnd(0, 359);
        L.has[i] = (uint8_t)(rnd(0, 9) < 8); L.obs[i] = rnd(0, 3);
        for (int c = 0; c < 3; ++c) L.xw[3 * (size_t)i + c] = (float)rnd(-50, 50) * 0.1f;
        for (int b = 0; b < 32; ++b) L.desc[(size_t)i * 32 + b] = (uint8_t)rnd(0, 255);
    }
    return L;
}
static Points make_points(int n, int nlevels) {
    Points M;
    M.in_view.resize(n); M.desc.resize((size_t)n * 32); M.proj.resize((size_t)n * 3); M.cosv.resize(n); M.level.resize(n); M.obs.resize(n);
    for (int i = 0; i < n; ++i) {
        M.in_view[i] = (uint8_t)(rnd(0, 9) < 8); M.level[i] = rnd(0, nlevels - 1); M.obs[i] = rnd(0, 3);
        M.cosv[i] = rnd(0, 1) ? 0.9999f : 0.99f;
        for (int c = 0; c < 3; ++c) M.proj[3 * (size_t)i + c] = (float)rnd(0, 200);
        for (int b = 0; b < 32; ++b) M.desc[(size_t)i * 32 + b] = (uint8_t)rnd(0, 255);
    }
    return M;
}

static uint64_t digest(const std::vector<uint8_t> &block) {   // reads every byte of the staging block
    uint64_t s = 1469598103934665603ull;
    for (uint8_t b : block) s = (s ^ b) * 1099511628211ull;
    return s;
}

int main() {
    const int nlevels = 8;
    float scale[16];
    scale[0] = 1.f;
    for (int i = 1; i < 16; ++i) scale[i] = scale[i - 1] * 1.2f;
    const char *why = "";
    OrbxTrackPlan plan;

    // ---- 0 problems
    { const OrbxTrackBatchArgs a = {4, 512, nlevels, true};
      CHECK(orbx_track_frame_plan(0, nullptr, a, plan, &why) == ORBX_OK && plan.nq == 0);
      CHECK(orbx_track_points_plan(0, nullptr, a, plan, &why) == ORBX_OK && plan.nq == 0);
      std::vector<uint8_t> block(plan.in_bytes);
      orbx_track_frame_pack(0, nullptr, plan, scale, 0.1f, block.data());
      orbx_track_points_pack(0, nullptr, plan, scale, 512, block.data());
      (void)digest(block); }

    // ---- the rejections
    { LastFrame L = make_last(10, nlevels);
      Points M = make_points(10, nlevels);
      orbx_track_frame_problem F; memset(&F, 0, sizeof(F)); F.th = 15.f; F.last = L.view();
      orbx_track_points_problem P; memset(&P, 0, sizeof(P)); P.th = 3.f; P.points = M.view();
      const OrbxTrackBatchArgs ok = {4, 512, nlevels, true};
      CHECK(orbx_track_frame_plan(1, &F, ok, plan, &why) == ORBX_OK && plan.nq == 10);
      CHECK(orbx_track_points_plan(1, &P, ok, plan, &why) == ORBX_OK && plan.nq == 10 && plan.seed_words == 16);
      CHECK(orbx_track_frame_plan(-1, &F, ok, plan, &why) == ORBX_BAD_ARGUMENT);
      CHECK(orbx_track_points_plan(-1, &P, ok, plan, &why) == ORBX_BAD_ARGUMENT);
      CHECK(orbx_track_frame_plan(1, nullptr, ok, plan, &why) == ORBX_BAD_ARGUMENT);
      CHECK(orbx_track_points_plan(1, nullptr, ok, plan, &why) == ORBX_BAD_ARGUMENT);
      const OrbxTrackBatchArgs cap0 = {4, 0, nlevels, true}, capbig = {4, 65536, nlevels, true}, nodev = {4, 512, nlevels, false};
      CHECK(orbx_track_frame_plan(1, &F, cap0, plan, &why) == ORBX_BAD_ARGUMENT);
      CHECK(orbx_track_points_plan(1, &P, cap0, plan, &why) == ORBX_BAD_ARGUMENT);
      CHECK(orbx_track_frame_plan(1, &F, capbig, plan, &why) == ORBX_UNSUPPORTED);
      CHECK(orbx_track_points_plan(1, &P, capbig, plan, &why) == ORBX_UNSUPPORTED);
      CHECK(orbx_track_frame_plan(1, &F, nodev, plan, &why) == ORBX_BAD_ARGUMENT);
      F.frame = 4; P.frame = -1;
      CHECK(orbx_track_frame_plan(1, &F, ok, plan, &why) == ORBX_BAD_ARGUMENT);
      CHECK(orbx_track_points_plan(1, &P, ok, plan, &why) == ORBX_BAD_ARGUMENT);
      F.frame = 3; P.frame = 0;
      CHECK(orbx_track_frame_plan(1, &F, ok, plan, &why) == ORBX_OK);
      L.keys[4].octave = nlevels; L.has[4] = 0;
      CHECK(orbx_track_frame_plan(1, &F, ok, plan, &why) == ORBX_OK);              // not a live point
      L.has[4] = 1;
      CHECK(orbx_track_frame_plan(1, &F, ok, plan, &why) == ORBX_BAD_ARGUMENT);
      L.keys[4].octave = -1;
      CHECK(orbx_track_frame_plan(1, &F, ok, plan, &why) == ORBX_BAD_ARGUMENT);
      M.level[7] = nlevels; M.in_view[7] = 0;
      CHECK(orbx_track_points_plan(1, &P, ok, plan, &why) == ORBX_OK);
      M.in_view[7] = 1;
      CHECK(orbx_track_points_plan(1, &P, ok, plan, &why) == ORBX_BAD_ARGUMENT);
      M.level[7] = 0;
      P.points.view_cos = nullptr;
      CHECK(orbx_track_points_plan(1, &P, ok, plan, &why) == ORBX_BAD_ARGUMENT);
      F.last.mp_desc = nullptr;
      CHECK(orbx_track_frame_plan(1, &F, ok, plan, &why) == ORBX_BAD_ARGUMENT);
      F.last.n = 0; P.points.n = 0;                                                // empty views: null fields are not read
      CHECK(orbx_track_frame_plan(1, &F, ok, plan, &why) == ORBX_OK && plan.nq == 0);
      CHECK(orbx_track_points_plan(1, &P, ok, plan, &why) == ORBX_OK && plan.nq == 0); }

    // ---- random batches: empty views, n == cap, NULL frame_observations; the block is exactly in_bytes long
    for (int round = 0; round < 200; ++round) {
        const int cap = round % 7 == 0 ? 1 : round % 5 == 0 ? 65535 : rnd(1, 700), K = rnd(1, 9), nframes = rnd(1, 5);
        const OrbxTrackBatchArgs a = {nframes, cap, nlevels, true};
        std::vector<LastFrame> Ls; std::vector<Points> Ms; std::vector<std::vector<int32_t>> fobs((size_t)K);
        std::vector<orbx_track_frame_problem> F((size_t)K); std::vector<orbx_track_points_problem> P((size_t)K);
        Ls.reserve(K); Ms.reserve(K);
        size_t nq = 0;
        for (int k = 0; k < K; ++k) {
            const int n = k % 4 == 1 ? 0 : k % 4 == 2 ? std::min(cap, 2000) : rnd(1, 400);   // empty, n == cap, anything
            nq += (size_t)n;
            Ls.push_back(make_last(n, nlevels)); Ms.push_back(make_points(n, nlevels));
            memset(&F[k], 0, sizeof(F[k])); memset(&P[k], 0, sizeof(P[k]));
            F[k].frame = rnd(0, nframes - 1); F[k].th = 15.f; F[k].mono = k & 1; F[k].last = Ls.back().view();
            for (int i = 0; i < 16; ++i) F[k].Tcw[i] = (i % 5 == 0) ? 1.f : 0.01f * (float)rnd(-9, 9);
            P[k].frame = rnd(0, nframes - 1); P[k].th = k % 3 ? 3.f : 1.f; P[k].points = Ms.back().view();
            if (k % 3 != 0) {                                                            // exactly cap entries, or NULL
                fobs[k].resize((size_t)cap);
                for (int i = 0; i < cap; ++i) fobs[k][i] = rnd(-1, 2);
                P[k].frame_observations = fobs[k].data();
            }
        }
        CHECK(orbx_track_frame_plan(K, F.data(), a, plan, &why) == ORBX_OK && plan.nq == nq);
        { std::vector<uint8_t> block(plan.in_bytes, 0xcd);
          orbx_track_frame_pack(K, F.data(), plan, scale, 0.1f, block.data());
          (void)digest(block);
          const DTrackProb *dp = (const DTrackProb *)(block.data() + plan.o_prob);
          const DTrackQ *dq = (const DTrackQ *)(block.data() + plan.o_q);
          size_t base = 0;
          for (int k = 0; k < K; ++k) {
              CHECK(dp[k].frame == F[k].frame && (size_t)dp[k].q_begin == base && dp[k].nq == F[k].last.n && dp[k].dir >= 0 && dp[k].dir <= 2);
              for (int i = 0; i < dp[k].nq; ++i) {
                  const DTrackQ &Q = dq[base + i];
                  CHECK(Q.prob == k && Q.obs == Ls[k].obs[i] && Q.min_level == Ls[k].keys[i].octave);
                  CHECK(Ls[k].has[i] ? Q.r == 15.f * scale[Q.min_level] : Q.r < 0.f);
              }
              if (dp[k].nq) CHECK(memcmp(block.data() + plan.o_desc + base * 32, Ls[k].desc.data(), (size_t)dp[k].nq * 32) == 0);
              base += (size_t)dp[k].nq;
          } }
        CHECK(orbx_track_points_plan(K, P.data(), a, plan, &why) == ORBX_OK && plan.nq == nq && plan.seed_words == (cap + 31) / 32);
        { std::vector<uint8_t> block(plan.in_bytes, 0xcd);
          orbx_track_points_pack(K, P.data(), plan, scale, cap, block.data());
          (void)digest(block);
          const DTrackProb *dp = (const DTrackProb *)(block.data() + plan.o_prob);
          const DTrackQ *dq = (const DTrackQ *)(block.data() + plan.o_q);
          const uint32_t *seed = (const uint32_t *)(block.data() + plan.o_seed);
          size_t base = 0;
          for (int k = 0; k < K; ++k) {
              CHECK(dp[k].frame == P[k].frame && (size_t)dp[k].q_begin == base && dp[k].nq == P[k].points.n);
              for (int i = 0; i < dp[k].nq; ++i) {
                  const DTrackQ &Q = dq[base + i];
                  CHECK(Q.prob == k && Q.obs == Ms[k].obs[i] && (Ms[k].in_view[i] ? Q.r > 0.f && Q.max_level == Ms[k].level[i] : Q.r < 0.f));
              }
              for (int i = 0; i < cap; ++i) {
                  const bool bit = (seed[(size_t)k * plan.seed_words + (i >> 5)] >> (i & 31)) & 1u;
                  CHECK(bit == (P[k].frame_observations != nullptr && fobs[k][i] > 0));
              }
              base += (size_t)dp[k].nq;
          } }
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
