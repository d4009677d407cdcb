// tests/san_pnp.cpp -- a stand-alone program around csrc/orbx_pnp.cpp (validation, packing, the host path, Refine, the cursor,
// append; HIP-free), built by tests/test_pnp_cpu.py with g++ -fsanitize=address,undefined: sizes around the mask words, every
// rejection, a replay that runs past the stored iterations and appends, a solver that launches nothing, non-finite input.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_pnp.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static uint64_t g_state = 1;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(g_state >> 33); }
static double uni(double a, double b) { return a + (b - a) * (rnd() / 2147483648.0); }

struct Scene {
    std::vector<float> p3, p2, me;
    std::vector<int32_t> sets;
    orbx_pnp_problem P;
};

// points 2 to 20 m in front of a camera at the identity, exact projections, every fifth point displaced
static void make(Scene &S, int n, int iterations, int min_inliers) {
    const double cam[4] = {517.3, 516.5, 318.6, 255.3};
    S.p3.resize((size_t)n * 3); S.p2.resize((size_t)n * 2); S.me.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        const double z = uni(2, 20), x = uni(-0.5, 0.5) * z, y = uni(-0.4, 0.4) * z;
        S.p3[3 * i] = (float)x; S.p3[3 * i + 1] = (float)y; S.p3[3 * i + 2] = (float)z;
        S.p2[2 * i] = (float)(cam[2] + cam[0] * x / z + (i % 5 == 4 ? 80.0 : 0.0));
        S.p2[2 * i + 1] = (float)(cam[3] + cam[1] * y / z);
        S.me[i] = 5.991f * (float)(1 + i % 3);
    }
    S.sets.resize((size_t)iterations * 4);
    for (int it = 0; it < iterations; ++it) {
        std::vector<int32_t> avail((size_t)n);
        for (int i = 0; i < n; ++i) avail[i] = i;
        for (int c = 0; c < 4 && !avail.empty(); ++c) {
            const size_t r = rnd() % avail.size();
            S.sets[4 * it + c] = avail[r];
            avail[r] = avail.back();
            avail.pop_back();
        }
    }
    S.P.n = n; S.P.p3dw = S.p3.data(); S.P.p2d = S.p2.data(); S.P.max_err = S.me.data();
    memcpy(S.P.camera, cam, sizeof(cam));
    S.P.min_inliers = min_inliers; S.P.iterations = iterations; S.P.sets = S.sets.data();
}

static orbx_pnp_batch *run(const std::vector<orbx_pnp_problem> &probs, orbx_status want = ORBX_OK) {
    OrbxPnpPlan plan;
    const char *why = "";
    const orbx_status st = orbx_pnp_plan((int)probs.size(), probs.data(), plan, &why);
    CHECK(st == want);
    if (st != ORBX_OK) return nullptr;
    orbx_pnp_batch *b = orbx_pnp_batch_new(probs.data(), plan);
    if (plan.nlaunch > 0) {
        std::vector<uint8_t> in(plan.in_bytes), out(plan.out_bytes);
        orbx_pnp_pack(probs.data(), plan, in.data());
        orbx_pnp_host_run(plan, in.data(), out.data());
        orbx_pnp_batch_take(b, plan, out.data());
    }
    return b;
}

// iterate(5) until the solver says no_more or 60 calls were made; a -2 is met with one more drawn set
static void replay(orbx_pnp_batch *b, int k, int n) {
    std::vector<uint8_t> inl((size_t)(n > 0 ? n : 1));
    float T[16];
    const char *why = "";
    int returned = 0;
    for (int call = 0; call < 60; ++call) {
        int32_t no_more = 0, nin = 0;
        int32_t r = orbx_pnp_cursor_iterate(b, k, 5, &no_more, inl.data(), &nin, T, &why);
        while (r == -2) {
            int32_t set[4] = {(int32_t)(rnd() % n), 0, 0, 0};
            for (int c = 1; c < 4; ++c) set[c] = (set[c - 1] + 1 + (int32_t)(rnd() % (n / 4))) % n;   // distinct for n >= 4
            CHECK(orbx_pnp_cursor_append(b, k, 1, set, &why) == ORBX_OK);
            r = orbx_pnp_cursor_iterate(b, k, 5, &no_more, inl.data(), &nin, T, &why);
        }
        CHECK(r == 0 || r == 1);
        if (r == 1) { ++returned; CHECK(nin > 0); }
        if (no_more) break;
    }
    (void)returned;
}

int main() {
    const int sizes[] = {4, 5, 63, 64, 65, 129, 513};
    std::vector<Scene> scenes(7);
    std::vector<orbx_pnp_problem> probs;
    for (int i = 0; i < 7; ++i) {
        make(scenes[i], sizes[i], i == 0 ? 1 : 9 + i, sizes[i] < 20 ? 4 : sizes[i] / 2);
        probs.push_back(scenes[i].P);
    }
    Scene few;                                                     // n < min_inliers: launches nothing, its sets are not read
    make(few, 6, 3, 10);
    few.P.sets = nullptr;
    probs.push_back(few.P);
    orbx_pnp_batch *b = run(probs);
    if (b) {
        const char *why = "";
        for (int k = 0; k < 7; ++k) {
            int32_t nit = 0;
            CHECK(orbx_pnp_cursor_counts(b, k, nullptr, &nit, &why) == ORBX_OK && nit == probs[k].iterations);
            std::vector<uint64_t> w((size_t)((sizes[k] + 63) / 64));
            double rt[12]; float T[16]; int32_t N = 0;
            CHECK(orbx_pnp_cursor_hypothesis(b, k, nit - 1, rt, T, &N, w.data(), &why) == ORBX_OK && N >= 1 && N <= 3);
            CHECK(orbx_pnp_cursor_hypothesis(b, k, nit, rt, T, &N, w.data(), &why) == ORBX_BAD_ARGUMENT);
            if (sizes[k] >= 8) replay(b, k, sizes[k]);
        }
        int32_t no_more = 0, nin = 0; uint8_t inl[8]; float T[16];
        CHECK(orbx_pnp_cursor_iterate(b, 7, 5, &no_more, inl, &nin, T, &why) == 0 && no_more == 1);
        CHECK(orbx_pnp_cursor_iterate(b, 8, 5, &no_more, inl, &nin, T, &why) == -1);
        CHECK(orbx_pnp_cursor_iterate(b, 0, 5, nullptr, inl, &nin, T, &why) == -1);
        int32_t set[4] = {0, 1, 2, 3};
        CHECK(orbx_pnp_cursor_append(b, 7, 1, set, &why) == ORBX_BAD_ARGUMENT);
        set[3] = 2;
        CHECK(orbx_pnp_cursor_append(b, 2, 1, set, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_pnp_cursor_best(b, 7, T, &nin, &nin, &why) == ORBX_BAD_ARGUMENT);
        delete b;
    }
    // rejections
    {
        Scene s; make(s, 12, 4, 6);
        std::vector<orbx_pnp_problem> one(1, s.P);
        one[0].n = -1; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].iterations = 0; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].p2d = nullptr; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].sets = nullptr; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        s.sets[5] = 12; run(one, ORBX_BAD_ARGUMENT);
        s.sets[5] = s.sets[4]; run(one, ORBX_BAD_ARGUMENT);
        OrbxPnpPlan plan; const char *why = "";
        CHECK(orbx_pnp_plan(-1, one.data(), plan, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_pnp_plan(1, nullptr, plan, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_pnp_plan(0, nullptr, plan, &why) == ORBX_OK && plan.nlaunch == 0);
    }
    // non-finite and degenerate input runs the same code
    {
        const float poison[] = {INFINITY, NAN, 1e30f, 0.0f};
        for (float v : poison) {
            Scene s; make(s, 24, 6, 8);
            s.p3[3 * s.sets[0]] = v; s.p3[3 * s.sets[0] + 1] = v; s.p3[3 * s.sets[0] + 2] = v;
            s.p2[2 * s.sets[9]] = v;
            std::vector<orbx_pnp_problem> one(1, s.P);
            orbx_pnp_batch *pb = run(one);
            if (pb) { replay(pb, 0, 24); delete pb; }
        }
        Scene flat; make(flat, 20, 5, 8);                           // exactly coplanar: CC is singular
        for (int i = 0; i < 20; ++i) flat.p3[3 * i + 2] = 5.0f;
        std::vector<orbx_pnp_problem> one(1, flat.P);
        orbx_pnp_batch *pb = run(one);
        if (pb) { replay(pb, 0, 20); delete pb; }
    }
    int32_t mi = 0, it = 0;
    for (int n = 0; n < 50; ++n) orbx_pnp_ransac_parameters(n, 0.99, 10, 300, 4, 0.5f, &mi, &it);
    CHECK(mi == 24 && it == 35);
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
