// san_pose_pack.cpp -- stand-alone driver of csrc/orbx_pose.cpp (the HIP-free validation, packing and host path of the batched
// Optimizer::PoseOptimization) for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_pose_batch_cpu.py builds and runs
// it).  Every caller array is an exactly sized heap block, so that a read or write past one is a report; the staging block is
// exactly plan.in_bytes long and is read back.  The host path runs on every edge count of the size list, on shared frames, on
// index lists, and on inputs outside the contract (z = 0, infinities, NaN), where it only has to come back.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_pose.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static std::mt19937 rng(23);
static float uni(float lo, float hi) { return lo + (hi - lo) * (float)(rng() >> 8) / 16777216.0f; }

struct Batch {
    int nframes, cap, nproblems, npool, nlevels = 8;
    std::vector<orbx_keypoint> keys;
    std::vector<float> ur, world, sig, T;
    std::vector<int32_t> counts, point, nin;
    std::vector<std::vector<int32_t>> index;
    std::vector<orbx_pose_problem> prob;
    std::vector<uint8_t> outlier;
    float cam[4] = {100.f, 100.f, 80.f, 60.f};
    OrbxPoseCall call() {
        OrbxPoseCall c;
        c.npool = npool; c.nframes = nframes; c.cap = cap; c.nlevels = nlevels;
        c.world_pos = world.data(); c.camera4 = cam; c.inv_level_sigma2 = sig.data(); c.mbf = 10.f;
        c.keys_un = keys.data(); c.u_right = ur.data(); c.counts = counts.data(); c.point = point.data();
        c.Tcw = T.data(); c.outlier = outlier.data(); c.ninliers = nin.data();
        return c;
    }
};

// identity pose as truth, start pose shifted; every frame has `cap` slots and counts[f] features, nedges[k] of them with a point
static Batch make(int nframes, int cap, const std::vector<int> &frame_of, const std::vector<int> &nedges, bool use_index) {
    Batch b;
    b.nframes = nframes; b.cap = cap; b.nproblems = (int)frame_of.size(); b.npool = cap + 3;
    b.keys.resize((size_t)nframes * cap); b.ur.resize((size_t)nframes * cap); b.counts.resize((size_t)nframes);
    b.world.resize((size_t)b.npool * 3); b.sig.resize(8);
    for (int l = 0; l < 8; ++l) b.sig[l] = 1.0f / (float)std::pow(1.44, l);
    // pool point j projects to feature j of every frame (plus noise per frame)
    for (int j = 0; j < b.npool; ++j) {
        const float z = uni(2.f, 10.f), u = uni(5.f, 155.f), v = uni(5.f, 115.f);
        b.world[3 * j] = (u - 80.f) / 100.f * z; b.world[3 * j + 1] = (v - 60.f) / 100.f * z; b.world[3 * j + 2] = z;
    }
    for (int f = 0; f < nframes; ++f) {
        b.counts[f] = cap - (f % 2);
        for (int i = 0; i < cap; ++i) {
            orbx_keypoint &k = b.keys[(size_t)f * cap + i];
            memset(&k, 0, sizeof(k));
            const float *P = &b.world[3 * i];
            k.x = 100.f * P[0] / P[2] + 80.f + uni(-1.f, 1.f); k.y = 100.f * P[1] / P[2] + 60.f + uni(-1.f, 1.f);
            k.octave = (int32_t)(rng() % 8);
            b.ur[(size_t)f * cap + i] = (rng() & 1) ? -1.f : k.x - 10.f / P[2];
        }
    }
    b.point.assign((size_t)b.nproblems * cap, -1);
    b.outlier.assign((size_t)b.nproblems * cap, 0x5A);
    b.T.assign((size_t)b.nproblems * 16, 77.f);
    b.nin.assign((size_t)b.nproblems, -5);
    b.index.resize((size_t)b.nproblems);
    b.prob.resize((size_t)b.nproblems);
    for (int k = 0; k < b.nproblems; ++k) {
        orbx_pose_problem &P = b.prob[k];
        memset(&P, 0, sizeof(P));
        P.frame = frame_of[k];
        const float T0[16] = {1, 0, 0, 0.02f * (k + 1), 0, 1, 0, -0.01f, 0, 0, 1, 0.03f, 0, 0, 0, 1};
        memcpy(P.Tcw, T0, sizeof(T0));
        const int n = b.counts[P.frame];
        int left = nedges[k];
        if (use_index) {                      // list position i -> pool index i, through an exactly sized list
            b.index[k].resize((size_t)n);
            for (int i = 0; i < n; ++i) b.index[k][i] = i;
            P.point_index = b.index[k].data(); P.npoints = n;
        } else {
            P.point_index = nullptr; P.npoints = b.npool;
        }
        for (int i = 0; i < n && left > 0; ++i)
            if (n - i <= left || (rng() % 3) != 0) { b.point[(size_t)k * cap + i] = i; --left; }
    }
    return b;
}

static void run_sizes() {
    const int sizes[] = {0, 2, 3, 9, 10, 63, 64, 65, 130, 256};
    for (int use_index = 0; use_index < 2; ++use_index) {
        std::vector<int> frame_of, nedges;
        for (int s : sizes) { frame_of.push_back((int)frame_of.size() % 3); nedges.push_back(s); }
        Batch b = make(3, 257, frame_of, nedges, use_index != 0);
        OrbxPoseCall c = b.call();
        OrbxPosePlan plan;
        const char *why = "";
        CHECK(orbx_pose_plan(b.nproblems, b.prob.data(), c, plan, &why) == ORBX_OK);
        CHECK(orbx_pose_check_rows(b.nproblems, b.prob.data(), c, &why) == ORBX_OK);
        CHECK(plan.in_bytes % 256 == 0);
        std::vector<uint8_t> block(plan.in_bytes, 0xEE);
        orbx_pose_pack(b.prob.data(), c, plan, block.data());
        const DPoseProb *dp = (const DPoseProb *)(block.data() + plan.o_prob);
        for (int k = 0; k < b.nproblems; ++k) {
            CHECK(dp[k].frame == b.prob[k].frame && dp[k].npoints == b.prob[k].npoints);
            CHECK(memcmp(dp[k].Tcw, b.prob[k].Tcw, 64) == 0);
            CHECK((dp[k].index_off >= 0) == (use_index != 0));
            if (use_index && b.prob[k].npoints > 0)
                CHECK(memcmp(block.data() + plan.o_index + 4 * (size_t)dp[k].index_off, b.prob[k].point_index, 4 * (size_t)b.prob[k].npoints) == 0);
        }
        CHECK(memcmp(block.data() + plan.o_world, b.world.data(), b.world.size() * 4) == 0);
        CHECK(memcmp(block.data() + plan.o_sig, b.sig.data(), 32) == 0);
        orbx_pose_host_run(b.nproblems, b.prob.data(), c);
        for (int k = 0; k < b.nproblems; ++k) {
            const int n = b.counts[b.prob[k].frame];
            int withpt = 0, bad = 0;
            for (int i = 0; i < b.cap; ++i) {
                const uint8_t o = b.outlier[(size_t)k * b.cap + i];
                const bool has = i < n && b.point[(size_t)k * b.cap + i] >= 0;
                if (has) { ++withpt; CHECK(o <= 1); bad += o; } else CHECK(o == 0x5A);      // only features with a point are written
            }
            CHECK(withpt == nedges[k]);
            if (nedges[k] < 3) { CHECK(b.nin[k] == 0 && b.T[16 * k] == 77.f && bad == 0); continue; }
            CHECK(b.nin[k] == withpt - bad);
            for (int j = 0; j < 16; ++j) CHECK(std::isfinite(b.T[16 * k + j]));
            if (nedges[k] >= 9) {               // noise of one pixel: the truth (identity) is recovered to a few centimetres
                CHECK(std::fabs(b.T[16 * k + 3]) < 0.08f && std::fabs(b.T[16 * k + 7]) < 0.08f && std::fabs(b.T[16 * k + 11]) < 0.15f);
                CHECK(b.nin[k] * 2 > withpt);
            }
        }
    }
}

static void run_outside_contract() {
    const float inf = INFINITY, nan = NAN;
    const float poison[][3] = {{0.f, 0.f, -0.03f}, {inf, 1.f, 2.f}, {nan, nan, nan}, {1e30f, -1e30f, 1e-30f}, {0.f, 0.f, 0.f}};
    for (const auto &p : poison)
        for (int many = 0; many < 2; ++many) {
            Batch b = make(1, 40, {0}, {30}, false);
            for (int i = 0; i < (many ? 40 : 1); ++i) memcpy(&b.world[3 * (size_t)(5 + i % 20)], p, 12);   // z = 0 in the camera frame for the first
            OrbxPoseCall c = b.call();
            orbx_pose_host_run(1, b.prob.data(), c);
            CHECK(b.nin[0] >= 0 && b.nin[0] <= 30);
        }
    Batch b = make(1, 40, {0}, {30}, false);          // a NaN pose and zero weights
    b.prob[0].Tcw[0] = nan;
    OrbxPoseCall c = b.call();
    orbx_pose_host_run(1, b.prob.data(), c);
    Batch z = make(1, 40, {0}, {30}, false);
    for (auto &s : z.sig) s = 0.f;
    OrbxPoseCall cz = z.call();
    orbx_pose_host_run(1, z.prob.data(), cz);
    CHECK(z.nin[0] == 30);                             // chi2 = 0 everywhere
    double s, cs;
    for (double th : {0.0, 1e-5, 0.5, 3.0, 1e6, 1073741823.9, 1073741824.0, 1e300, (double)inf, (double)nan}) {
        orbx_pose_sincos(th, &s, &cs);
        CHECK(std::fabs(s) <= 1.0000001 && std::fabs(cs) <= 1.0000001);
    }
}

static void run_rejections() {
    Batch b = make(2, 16, {0, 1}, {8, 8}, true);
    OrbxPoseCall c = b.call();
    OrbxPosePlan plan;
    const char *why = "";
    auto P = [&](int n, const OrbxPoseCall &cc) { return orbx_pose_plan(n, b.prob.data(), cc, plan, &why); };
    CHECK(P(2, c) == ORBX_OK);
    CHECK(P(-1, c) == ORBX_BAD_ARGUMENT);
    CHECK(orbx_pose_plan(2, nullptr, c, plan, &why) == ORBX_BAD_ARGUMENT);
    { OrbxPoseCall d = c; d.cap = 0; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); CHECK(P(0, d) == ORBX_BAD_ARGUMENT); }
    { OrbxPoseCall d = c; d.cap = 65536; CHECK(P(2, d) == ORBX_UNSUPPORTED); }
    { OrbxPoseCall d = c; d.cap = 65535; CHECK(P(2, d) == ORBX_OK); }
    { OrbxPoseCall d = c; d.nframes = 1; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); }
    { OrbxPoseCall d = c; d.npool = 3; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); }              // index 3.. outside a pool of 3
    { OrbxPoseCall d = c; d.nlevels = 0; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); }
    { OrbxPoseCall d = c; d.keys_un = nullptr; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); }
    { OrbxPoseCall d = c; d.counts = nullptr; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); }
    { OrbxPoseCall d = c; d.point = nullptr; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); }
    { OrbxPoseCall d = c; d.Tcw = nullptr; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); }
    { OrbxPoseCall d = c; d.outlier = nullptr; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); }
    { OrbxPoseCall d = c; d.ninliers = nullptr; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); }
    { OrbxPoseCall d = c; d.camera4 = nullptr; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); }
    { OrbxPoseCall d = c; d.inv_level_sigma2 = nullptr; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); }
    { OrbxPoseCall d = c; d.world_pos = nullptr; CHECK(P(2, d) == ORBX_BAD_ARGUMENT); }
    { OrbxPoseCall d = c; d.u_right = nullptr; CHECK(P(2, d) == ORBX_OK); }                // all monocular
    CHECK(P(0, c) == ORBX_OK && plan.in_bytes == 0);
    b.prob[1].frame = 2; CHECK(P(2, c) == ORBX_BAD_ARGUMENT); b.prob[1].frame = -1; CHECK(P(2, c) == ORBX_BAD_ARGUMENT); b.prob[1].frame = 1;
    b.prob[1].npoints = -1; CHECK(P(2, c) == ORBX_BAD_ARGUMENT); b.prob[1].npoints = (int)b.index[1].size();
    b.index[1][3] = b.npool; CHECK(P(2, c) == ORBX_BAD_ARGUMENT); b.index[1][3] = -1; CHECK(P(2, c) == ORBX_BAD_ARGUMENT); b.index[1][3] = 3;
    { const int32_t *keep = b.prob[0].point_index; b.prob[0].point_index = nullptr; b.prob[0].npoints = b.npool + 1;
      CHECK(P(2, c) == ORBX_BAD_ARGUMENT); b.prob[0].npoints = b.npool; CHECK(P(2, c) == ORBX_OK);
      b.prob[0].point_index = keep; b.prob[0].npoints = (int)b.index[0].size(); }
    CHECK(P(2, c) == ORBX_OK);
    // host rows
    CHECK(orbx_pose_check_rows(2, b.prob.data(), c, &why) == ORBX_OK);
    int slot = -1;
    for (int i = 0; i < 15; ++i) if (b.point[16 + i] >= 0) slot = i;
    CHECK(slot >= 0);
    const int32_t keep = b.point[16 + slot];
    b.point[16 + slot] = b.prob[1].npoints; CHECK(orbx_pose_check_rows(2, b.prob.data(), c, &why) == ORBX_BAD_ARGUMENT); b.point[16 + slot] = keep;
    b.keys[16 + slot].octave = 8; CHECK(orbx_pose_check_rows(2, b.prob.data(), c, &why) == ORBX_BAD_ARGUMENT);
    b.keys[16 + slot].octave = -1; CHECK(orbx_pose_check_rows(2, b.prob.data(), c, &why) == ORBX_BAD_ARGUMENT);
    b.point[16 + slot] = -1; CHECK(orbx_pose_check_rows(2, b.prob.data(), c, &why) == ORBX_OK);   // no point there: the octave is not read
}

// orbx_debug_pose_inlier_test's form: two poses per problem packed behind the level table, the inlier test alone
static void run_inlier_test_form() {
    Batch b = make(2, 70, {0, 1, 0}, {65, 9, 0}, true);
    std::vector<float> est, last;
    for (int k = 0; k < b.nproblems; ++k)
        for (int j = 0; j < 16; ++j) { est.push_back(j % 5 == 0 ? 1.f : 0.f); last.push_back(b.prob[k].Tcw[j]); }
    for (auto &o : b.outlier) o = (uint8_t)(rng() & 1);
    OrbxPoseCall c = b.call();
    c.dbg_est = est.data(); c.dbg_last = last.data();
    OrbxPosePlan plan;
    const char *why = "";
    CHECK(orbx_pose_plan(b.nproblems, b.prob.data(), c, plan, &why) == ORBX_OK);
    CHECK(plan.in_bytes == plan.o_dbg + 512);
    std::vector<uint8_t> block(plan.in_bytes, 0xEE);
    orbx_pose_pack(b.prob.data(), c, plan, block.data());
    CHECK(memcmp(block.data() + plan.o_dbg, est.data(), est.size() * 4) == 0);
    CHECK(memcmp(block.data() + plan.o_dbg + est.size() * 4, last.data(), last.size() * 4) == 0);
    orbx_pose_host_run(b.nproblems, b.prob.data(), c);
    CHECK(b.T[0] == 77.f && b.nin[0] >= 0 && b.nin[0] <= 65 && b.nin[1] <= 9 && b.nin[2] == 0);
    { OrbxPoseCall d = c; d.dbg_last = nullptr; CHECK(orbx_pose_plan(b.nproblems, b.prob.data(), d, plan, &why) == ORBX_BAD_ARGUMENT); }
}

int main() {
    run_rejections();
    run_sizes();
    run_outside_contract();
    run_inlier_test_form();
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
