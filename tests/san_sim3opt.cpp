// san_sim3opt.cpp -- stand-alone driver of csrc/orbx_sim3opt.cpp (the HIP-free validation, packing, host path and scatter of the
// batched Optimizer::OptimizeSim3) for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_sim3opt_cpu.py builds and runs
// it).  Every caller array is an exactly sized heap block, so that a read or write past one is a report; the staging blocks are
// exactly plan.in_bytes and plan.out_bytes long.  The host path runs on every size of the size list with fix_scale 0 and 1 in
// one batch, the inlier test alone, every rejection, and inputs outside the contract (z = 0, infinities, NaN, s = 0), where it
// only has to come back with canonical NaNs.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_sim3opt.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static std::mt19937 rng(29);
static float uni(float lo, float hi) { return lo + (hi - lo) * (float)(rng() >> 8) / 16777216.0f; }

struct Scene {
    std::vector<float> x1, x2, o1, o2, w1, w2;
    std::vector<uint8_t> keep;
    orbx_sim3opt_problem P;
};
// truth: x1 = 1.1 * x2 + (0.1, -0.05, 0.2), no rotation; start: identity rotation, t = 0, s = 1
static void make(Scene &S, int n, int fix_scale) {
    S.x1.resize(3 * (size_t)n); S.x2.resize(3 * (size_t)n); S.o1.resize(2 * (size_t)n); S.o2.resize(2 * (size_t)n);
    S.w1.resize((size_t)n); S.w2.resize((size_t)n); S.keep.assign((size_t)n, 0xA5);
    const float sc = fix_scale ? 1.0f : 1.1f;
    for (int i = 0; i < n; ++i) {
        float *a = &S.x1[3 * (size_t)i], *b = &S.x2[3 * (size_t)i];
        a[0] = uni(-1.5f, 1.5f); a[1] = uni(-1.f, 1.f); a[2] = uni(2.5f, 8.f);
        b[0] = (a[0] - 0.1f) / sc; b[1] = (a[1] + 0.05f) / sc; b[2] = (a[2] - 0.2f) / sc;
        const float gross = (rng() % 8 == 0) ? 40.f : 0.f;
        S.o1[2 * (size_t)i] = 500.f * a[0] / a[2] + 320.f + uni(-1.f, 1.f) + gross; S.o1[2 * (size_t)i + 1] = 510.f * a[1] / a[2] + 240.f + uni(-1.f, 1.f);
        S.o2[2 * (size_t)i] = 520.f * b[0] / b[2] + 310.f + uni(-1.f, 1.f); S.o2[2 * (size_t)i + 1] = 530.f * b[1] / b[2] + 250.f + uni(-1.f, 1.f);
        S.w1[(size_t)i] = 1.0f / (float)std::pow(1.44, (double)(rng() % 8)); S.w2[(size_t)i] = 1.0f / (float)std::pow(1.44, (double)(rng() % 8));
    }
    orbx_sim3opt_problem &P = S.P;
    memset(&P, 0, sizeof(P));
    P.n = n;
    P.x1c = S.x1.data(); P.x2c = S.x2.data(); P.obs1 = S.o1.data(); P.obs2 = S.o2.data();
    P.inv_sigma2_1 = S.w1.data(); P.inv_sigma2_2 = S.w2.data(); P.keep = S.keep.data();
    const float c1[4] = {500.f, 510.f, 320.f, 240.f}, c2[4] = {520.f, 530.f, 310.f, 250.f};
    memcpy(P.camera1, c1, sizeof(c1)); memcpy(P.camera2, c2, sizeof(c2));
    P.R[0] = P.R[4] = P.R[8] = 1.f; P.s = 1.f; P.th2 = 10.f; P.fix_scale = fix_scale;
}

static bool canonical(const orbx_sim3opt_result &r) {
    const double *d = r.r;      // r[4], t[3], s are laid out one after the other
    for (int i = 0; i < 8; ++i) { uint64_t b; memcpy(&b, &d[i], 8); if (d[i] != d[i] && b != 0x7ff8000000000000ull) return false; }
    for (int i = 0; i < 16; ++i) { uint32_t b; memcpy(&b, &r.T12[i], 4); if (r.T12[i] != r.T12[i] && b != 0x7fc00000u) return false; }
    return true;
}

// plan, pack, run and scatter through exactly sized blocks
static orbx_status run(std::vector<orbx_sim3opt_problem> &probs, std::vector<orbx_sim3opt_result> &res, const double *last, bool test_only) {
    OrbxSim3OptPlan plan;
    const char *why = "";
    const orbx_status st = orbx_sim3opt_plan((int)probs.size(), probs.data(), res.data(), last, test_only, plan, &why);
    if (st != ORBX_OK || probs.empty()) return st;
    uint8_t *in = (uint8_t *)malloc(plan.in_bytes), *out = (uint8_t *)malloc(plan.out_bytes);
    memset(in, 0, plan.in_bytes);
    orbx_sim3opt_pack(probs.data(), last, plan, in);
    orbx_sim3opt_host_run(plan, in, test_only, out);
    orbx_sim3opt_unpack(probs.data(), plan, out, res.data());
    free(in); free(out);
    return st;
}

int main() {
    const int sizes[] = {0, 1, 9, 10, 11, 19, 20, 63, 64, 65, 129};
    std::vector<Scene> scenes(22);
    std::vector<orbx_sim3opt_problem> probs;
    for (int k = 0; k < 22; ++k) { make(scenes[k], sizes[k / 2], k & 1); probs.push_back(scenes[k].P); }
    std::vector<orbx_sim3opt_result> res(22);
    CHECK(run(probs, res, nullptr, false) == ORBX_OK);
    for (int k = 0; k < 22; ++k) {
        const int n = sizes[k / 2];
        int kept = 0;
        for (int i = 0; i < n; ++i) { CHECK(scenes[k].keep[i] <= 1); kept += scenes[k].keep[i]; }
        CHECK(res[k].ncorr == n && canonical(res[k]));
        CHECK(res[k].written == (n - res[k].nbad >= 10 ? 1 : 0));
        CHECK(res[k].ninliers == (res[k].written ? kept : 0));
        if (n >= 19) CHECK(res[k].written == 1 && res[k].ninliers >= n / 2);
        if (k & 1) CHECK(res[k].s == 1.0);
    }
    {   // the inlier test alone
        std::vector<double> last(8 * 22, 0.0);
        for (int k = 0; k < 22; ++k) { last[8 * k + 3] = 1.0; last[8 * k + 7] = 1.0; }
        CHECK(run(probs, res, last.data(), true) == ORBX_OK);
        for (int k = 0; k < 22; ++k) CHECK(res[k].written == 0 && res[k].ninliers + res[k].nbad == sizes[k / 2]);
    }
    {   // every rejection
        OrbxSim3OptPlan plan;
        const char *why = "";
        double last[8] = {0};
        CHECK(orbx_sim3opt_plan(-1, probs.data(), res.data(), nullptr, false, plan, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_sim3opt_plan(2, nullptr, res.data(), nullptr, false, plan, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_sim3opt_plan(2, probs.data(), nullptr, nullptr, false, plan, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_sim3opt_plan(2, probs.data(), res.data(), nullptr, true, plan, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_sim3opt_plan(0, nullptr, nullptr, nullptr, false, plan, &why) == ORBX_OK && plan.nproblems == 0);
        CHECK(orbx_sim3opt_plan(0, nullptr, nullptr, last, true, plan, &why) == ORBX_OK);
        std::vector<orbx_sim3opt_problem> bad(probs.begin() + 4, probs.begin() + 8);
        bad[1].n = -1; CHECK(orbx_sim3opt_plan(4, bad.data(), res.data(), nullptr, false, plan, &why) == ORBX_BAD_ARGUMENT);
        bad[1].n = probs[5].n;
        const float **fp[] = {&bad[2].x1c, &bad[2].x2c, &bad[2].obs1, &bad[2].obs2, &bad[2].inv_sigma2_1, &bad[2].inv_sigma2_2};
        for (const float **p : fp) {
            const float *was = *p;
            *p = nullptr; CHECK(orbx_sim3opt_plan(4, bad.data(), res.data(), nullptr, false, plan, &why) == ORBX_BAD_ARGUMENT);
            *p = was;
        }
        uint8_t *was = bad[2].keep;
        bad[2].keep = nullptr; CHECK(orbx_sim3opt_plan(4, bad.data(), res.data(), nullptr, false, plan, &why) == ORBX_BAD_ARGUMENT);
        bad[2].keep = was;
        CHECK(orbx_sim3opt_plan(4, bad.data(), res.data(), nullptr, false, plan, &why) == ORBX_OK);
        orbx_sim3opt_problem empty;                              // n == 0 reads no array
        memset(&empty, 0, sizeof(empty));
        CHECK(orbx_sim3opt_plan(1, &empty, res.data(), nullptr, false, plan, &why) == ORBX_OK && plan.total == 0);
    }
    {   // outside the contract: the call ends, stored NaNs are canonical
        const float inf = INFINITY, nan = NAN;
        const float poison[][3] = {{inf, 1.f, 2.f}, {nan, nan, nan}, {1e30f, -1e30f, 1e-30f}, {0.5f, -0.25f, 0.f}};
        std::vector<Scene> sc(9);
        std::vector<orbx_sim3opt_problem> pr;
        for (int k = 0; k < 9; ++k) make(sc[k], 30 + k, k & 1);
        for (int k = 0; k < 4; ++k) { memcpy(&sc[k].x2[0], poison[k], 12); memcpy(&sc[k].x1[15], poison[k], 12); }
        sc[4].P.s = 0.f;
        sc[5].P.s = nan;
        sc[6].P.th2 = nan;
        for (auto &w : sc[7].w1) w = 0.f;
        for (auto &w : sc[7].w2) w = 0.f;
        sc[8].o1[14] = nan; sc[8].o2[3] = inf; sc[8].P.R[0] = inf;
        for (auto &s : sc) pr.push_back(s.P);
        std::vector<orbx_sim3opt_result> r(9);
        CHECK(run(pr, r, nullptr, false) == ORBX_OK);
        for (int k = 0; k < 9; ++k) { CHECK(canonical(r[k]) && r[k].ncorr == 30 + k); for (uint8_t b : sc[k].keep) CHECK(b <= 1); }
        CHECK(r[5].s != r[5].s);
    }
    {   // the exp primitive at its edges
        CHECK(orbx_sim3opt_expd(0.0) == 1.0 && orbx_sim3opt_expd(709.5) == INFINITY && orbx_sim3opt_expd(-708.5) == 0.0);
        CHECK(orbx_sim3opt_expd(709.0) > 8e307 && orbx_sim3opt_expd(-708.0) > 0.0 && orbx_sim3opt_expd(NAN) != orbx_sim3opt_expd(NAN));
        CHECK(std::fabs(orbx_sim3opt_expd(1.0) - std::exp(1.0)) <= 4.5e-16);
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
