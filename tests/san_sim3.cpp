// san_sim3.cpp -- stand-alone driver of csrc/orbx_sim3.cpp (the HIP-free validation, packing, host path and iterate cursor of the
// batched Sim3Solver RANSAC) for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_sim3_cpu.py builds and runs it).
// Every caller array is an exactly sized heap block, so that a read or write past one is a report; the staging block is exactly
// plan.in_bytes long and the result block exactly plan.out_bytes.  The host path runs on sizes around the 64-point mask words,
// on mixed calls with problems that launch nothing, on every rejection, and on degenerate and non-finite input, where it only
// has to come back.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_sim3.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static std::mt19937 rng(29);
static float uni(float lo, float hi) { return lo + (hi - lo) * (float)(rng() >> 8) / 16777216.0f; }

struct Prob {
    std::vector<float> x1, x2, e1, e2;
    std::vector<int32_t> sets;
    orbx_sim3_problem p;
};
// x1 = 1.2 x2 + (0.1, -0.2, 0.3) plus a little noise; every fourth correspondence is an outlier
static Prob *make(int n, int iterations, int min_inliers, int fix_scale) {
    Prob *q = new Prob();
    q->x1.resize((size_t)n * 3); q->x2.resize((size_t)n * 3); q->e1.resize((size_t)n); q->e2.resize((size_t)n);
    q->sets.resize((size_t)iterations * 3);
    for (int i = 0; i < n; ++i) {
        const float X = uni(-1.5f, 1.5f), Y = uni(-1.f, 1.f), Z = uni(3.f, 7.f);
        q->x2[3 * i] = X; q->x2[3 * i + 1] = Y; q->x2[3 * i + 2] = Z;
        q->x1[3 * i] = 1.2f * X + 0.1f + uni(-1e-3f, 1e-3f); q->x1[3 * i + 1] = 1.2f * Y - 0.2f; q->x1[3 * i + 2] = 1.2f * Z + 0.3f;
        if (i % 4 == 3) q->x1[3 * i] += 1.0f;
        q->e1[i] = 9.21f * (float)std::pow(1.44, (double)(rng() % 8)); q->e2[i] = 9.21f;
    }
    for (size_t i = 0; i < q->sets.size(); ++i) q->sets[i] = n > 0 ? (int32_t)(rng() % (unsigned)n) : 0;
    orbx_sim3_problem &p = q->p;
    p.n = n;
    p.x1c = n ? q->x1.data() : nullptr; p.x2c = n ? q->x2.data() : nullptr;
    p.max_err1 = n ? q->e1.data() : nullptr; p.max_err2 = n ? q->e2.data() : nullptr;
    const float K1[4] = {500.f, 505.f, 320.f, 240.f}, K2[4] = {520.f, 515.f, 310.f, 250.f};
    memcpy(p.camera1, K1, sizeof(K1)); memcpy(p.camera2, K2, sizeof(K2));
    p.fix_scale = fix_scale; p.min_inliers = min_inliers; p.iterations = iterations;
    p.sets = q->sets.data();
    return q;
}

// plan, pack into an exactly sized block, host path into an exactly sized block, replay every solver to exhaustion
static orbx_status run(const std::vector<Prob *> &ps, bool expect_inliers) {
    std::vector<orbx_sim3_problem> arr;
    for (Prob *q : ps) arr.push_back(q->p);
    OrbxSim3Plan plan;
    const char *why = "";
    const orbx_status st = orbx_sim3_plan((int)arr.size(), arr.data(), plan, &why);
    if (st != ORBX_OK) return st;
    uint8_t *in = (uint8_t *)malloc(plan.in_bytes ? plan.in_bytes : 1);
    memset(in, 0xA5, plan.in_bytes);
    orbx_sim3_pack(arr.data(), plan, in);
    orbx_sim3_batch *b = orbx_sim3_batch_new(arr.data(), plan);
    CHECK(b->out.size() == (plan.nlaunch ? plan.out_bytes : 0));
    if (plan.nlaunch) orbx_sim3_host_run(plan, in, b->out.data());
    free(in);
    int best_total = 0;
    for (int k = 0; k < (int)arr.size(); ++k) {
        const int n = arr[k].n;
        uint8_t *inl = (uint8_t *)malloc(n ? n : 1);
        int32_t *counts = (int32_t *)malloc(sizeof(int32_t) * arr[k].iterations);
        uint64_t *words = (uint64_t *)malloc(sizeof(uint64_t) * ((n + 63) / 64 ? (n + 63) / 64 : 1));
        float T[16], R[9], t[3], s, h48[48];
        int32_t nit = -1, no_more = 0, nin = 0, calls = 0, returned = 0;
        CHECK(orbx_sim3_cursor_counts(b, k, counts, &nit, &why) == ORBX_OK);
        CHECK(nit == (n >= arr[k].min_inliers ? arr[k].iterations : 0));
        for (int i = 0; i < nit; ++i) {
            CHECK(counts[i] >= 0 && counts[i] <= n);
            CHECK(orbx_sim3_cursor_hypothesis(b, k, i, h48, words, &why) == ORBX_OK);
            int pop = 0;
            for (int w = 0; w < (n + 63) / 64; ++w) pop += __builtin_popcountll(words[w]);
            CHECK(pop == counts[i]);
            if (n % 64) CHECK((words[(n - 1) / 64] >> (n % 64)) == 0);     // no bit past the last correspondence
        }
        CHECK(orbx_sim3_cursor_hypothesis(b, k, nit, h48, words, &why) == ORBX_BAD_ARGUMENT);
        while (!no_more && calls < 1000) {
            const int32_t r = orbx_sim3_cursor_iterate(b, k, 5, &no_more, inl, &nin, T, &why);
            CHECK(r == 0 || r == 1);
            ++calls;
            if (r == 1) {
                ++returned;
                int c = 0;
                for (int i = 0; i < n; ++i) c += inl[i];
                CHECK(c == nin && nin > arr[k].min_inliers);
                CHECK(orbx_sim3_cursor_best(b, k, R, t, &s, &why) == ORBX_OK);
                CHECK(T[0] == s * R[0] && T[3] == t[0]);
            }
        }
        CHECK(no_more && calls <= arr[k].iterations + 1);
        best_total += returned;
        CHECK(orbx_sim3_cursor_iterate(b, k, 5, &no_more, inl, &nin, T, &why) == 0 && no_more);
        free(inl); free(counts); free(words);
    }
    if (expect_inliers) CHECK(best_total > 0);
    float T[16]; int32_t a, c; uint8_t d;
    CHECK(orbx_sim3_cursor_iterate(b, (int)arr.size(), 5, &a, &d, &c, T, &why) == -1);
    CHECK(orbx_sim3_cursor_iterate(b, -1, 5, &a, &d, &c, T, &why) == -1);
    delete b;
    return ORBX_OK;
}

int main() {
    // sizes around the mask words and the LDS chunk, iteration counts around the workgroup size
    for (int n : {3, 20, 63, 64, 65, 129, 511, 512, 513})
        for (int it : {1, 5, 64, 65}) {
            std::vector<Prob *> ps = {make(n, it, n < 20 ? 3 : 6, (n + it) & 1)};
            CHECK(run(ps, false) == ORBX_OK);
            delete ps[0];
        }
    {   // a mixed call: two that launch nothing (one with no sets at all), n = 0, and the RANSAC succeeding
        std::vector<Prob *> ps = {make(100, 300, 20, 0), make(10, 7, 20, 0), make(0, 3, 20, 0), make(65, 40, 6, 1), make(5, 2, 6, 0)};
        ps[4]->p.sets = nullptr;
        CHECK(run(ps, true) == ORBX_OK);
        CHECK(run({}, false) == ORBX_OK);
        // every rejection
        OrbxSim3Plan plan; const char *why = "";
        CHECK(orbx_sim3_plan(-1, nullptr, plan, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_sim3_plan(1, nullptr, plan, &why) == ORBX_BAD_ARGUMENT);
        Prob *q = ps[0];
        q->p.n = -1; CHECK(run(ps, false) == ORBX_BAD_ARGUMENT); q->p.n = 100;
        q->p.iterations = 0; CHECK(run(ps, false) == ORBX_BAD_ARGUMENT); q->p.iterations = 300;
        q->p.x1c = nullptr; CHECK(run(ps, false) == ORBX_BAD_ARGUMENT); q->p.x1c = q->x1.data();
        q->p.max_err2 = nullptr; CHECK(run(ps, false) == ORBX_BAD_ARGUMENT); q->p.max_err2 = q->e2.data();
        q->p.sets = nullptr; CHECK(run(ps, false) == ORBX_BAD_ARGUMENT); q->p.sets = q->sets.data();
        q->sets[899] = 100; CHECK(run(ps, false) == ORBX_BAD_ARGUMENT);
        q->sets[899] = -1; CHECK(run(ps, false) == ORBX_BAD_ARGUMENT);
        q->sets[899] = 99; CHECK(run(ps, false) == ORBX_OK);
        for (Prob *p : ps) delete p;
    }
    {   // outside the contract: one point three times, collinear points, z = 0, infinities, NaN, huge values
        Prob *q = make(40, 12, 6, 0);
        q->sets[0] = q->sets[1] = q->sets[2] = 4;
        q->sets[3] = 4; q->sets[4] = 4; q->sets[5] = 7;
        for (int c = 0; c < 3; ++c) { q->x2[3 + c] = 0.5f * (q->x2[c] + q->x2[6 + c]); q->x1[3 + c] = 0.5f * (q->x1[c] + q->x1[6 + c]); }
        q->sets[6] = 0; q->sets[7] = 1; q->sets[8] = 2;
        q->x1[3 * 10 + 2] = 0.f;
        q->x2[3 * 11] = INFINITY; q->x1[3 * 12 + 1] = NAN; q->x2[3 * 13 + 2] = 1e30f; q->x1[3 * 14] = -1e38f;
        q->sets[9] = 11; q->sets[12] = 12; q->sets[15] = 13; q->sets[18] = 14;
        std::vector<Prob *> ps = {q};
        CHECK(run(ps, false) == ORBX_OK);
        q->p.fix_scale = 1;
        CHECK(run(ps, false) == ORBX_OK);
        delete q;
    }
    // SetRansacParameters at its edges: n = 0 (epsilon is inf or NaN), probability 1 and 0, epsilon^3 that rounds 1 - x to 1
    for (int n : {0, 1, 20, 21, 100, 1000000})
        for (double pr : {0.99, 1.0, 0.0, 0.5})
            for (int mi : {0, 6, 20})
                for (int mx : {0, 1, 300}) { const int32_t r = orbx_sim3_ransac_iterations(n, pr, mi, mx); CHECK(r >= 1 && (r <= mx || r == 1)); }
    CHECK(orbx_sim3_ransac_iterations(20, 0.99, 20, 300) == 1);
    CHECK(orbx_sim3_atan2(0.0, 1.0) == 0.0 && std::isnan(orbx_sim3_atan2(NAN, 1.0)));
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
