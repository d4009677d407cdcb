// tests/san_init.cpp -- a stand-alone program around csrc/orbx_init.cpp (validation, Normalize, packing, the host path, the result
// object; HIP-free), built by tests/test_init_cpu.py with g++ -fsanitize=address,undefined: sizes around the mask words, every
// rejection, problems that launch nothing, degenerate sets and non-finite input.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_init.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static uint64_t g_state = 1;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(g_state >> 33); }
static double uni(double a, double b) { return a + (b - a) * (rnd() / 2147483648.0); }

struct Scene {
    std::vector<float> k1, k2;
    std::vector<int32_t> matches, sets;
    orbx_init_problem P;
};

// a plane seen from two cameras (a fixed homography), every fifth match displaced by 40 px; extra unmatched keypoints in both
// frames; match i pairs keypoint n1 - 1 - i of frame 1 with keypoint i of frame 2
static void make(Scene &S, int n, int iterations, int models, int extra1 = 3, int extra2 = 5) {
    const double Hm[9] = {0.98, 0.03, 12.0, -0.02, 1.01, -7.0, 1e-5, -2e-5, 1.0};
    const int n1 = n + extra1, n2 = n + extra2;
    S.k1.resize((size_t)n1 * 2); S.k2.resize((size_t)n2 * 2);
    for (int i = 0; i < n1; ++i) { S.k1[2 * i] = (float)uni(10, 630); S.k1[2 * i + 1] = (float)uni(10, 470); }
    for (int i = 0; i < n2; ++i) { S.k2[2 * i] = (float)uni(10, 630); S.k2[2 * i + 1] = (float)uni(10, 470); }
    S.matches.resize((size_t)n * 2);
    for (int i = 0; i < n; ++i) {
        const int a = n1 - 1 - i;
        const double x = S.k1[2 * a], y = S.k1[2 * a + 1], w = Hm[6] * x + Hm[7] * y + Hm[8];
        S.k2[2 * i] = (float)((Hm[0] * x + Hm[1] * y + Hm[2]) / w + (i % 5 == 4 ? 40.0 : 0.0));
        S.k2[2 * i + 1] = (float)((Hm[3] * x + Hm[4] * y + Hm[5]) / w);
        S.matches[2 * i] = a; S.matches[2 * i + 1] = i;
    }
    S.sets.resize((size_t)iterations * 8);
    for (int it = 0; it < iterations && n >= 8; ++it) {
        std::vector<int32_t> avail((size_t)n);
        for (int i = 0; i < n; ++i) avail[i] = i;
        for (int c = 0; c < 8; ++c) {
            const size_t r = rnd() % avail.size();
            S.sets[8 * it + c] = avail[r];
            avail[r] = avail.back();
            avail.pop_back();
        }
    }
    S.P.n1 = n1; S.P.n2 = n2; S.P.keys1 = S.k1.data(); S.P.keys2 = S.k2.data();
    S.P.n = n; S.P.matches = S.matches.data(); S.P.sigma = 1.0f; S.P.iterations = iterations; S.P.sets = S.sets.data();
    S.P.models = models;
}

static orbx_init_batch *run(const std::vector<orbx_init_problem> &probs, orbx_status want = ORBX_OK) {
    OrbxInitPlan plan;
    const char *why = "";
    const orbx_status st = orbx_init_plan((int)probs.size(), probs.data(), plan, &why);
    CHECK(st == want);
    if (st != ORBX_OK) return nullptr;
    orbx_init_batch *b = orbx_init_batch_new(probs.data(), plan);
    if (plan.nlaunch > 0) {
        std::vector<uint8_t> in(plan.in_bytes), out(plan.out_bytes);
        orbx_init_pack(probs.data(), plan, in.data());
        orbx_init_host_run(plan, in.data(), out.data());
        orbx_init_batch_take(b, plan, out.data());
    }
    return b;
}

// every accessor of problem k into buffers of exactly the documented sizes
static int32_t read_all(orbx_init_batch *b, int k, const orbx_init_problem &P) {
    const char *why = "";
    const size_t n = (size_t)P.n, nw = (size_t)((P.n + 63) / 64);
    std::vector<uint8_t> iH(n), iF(n);
    std::vector<uint64_t> w(nw);
    float SH, SF, RH, H[9], Fm[9], T1[9], T2[9], M[9], Mi[9], s;
    int32_t itH, itF, model, nit;
    CHECK(orbx_init_get_result(b, k, &SH, &SF, H, Fm, n ? iH.data() : nullptr, n ? iF.data() : nullptr, &itH, &itF, &RH, &model, &why) == ORBX_OK);
    CHECK(orbx_init_get_result(b, k, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &why) == ORBX_OK);
    CHECK(orbx_init_get_normalization(b, k, T1, T2, &why) == ORBX_OK);
    for (int model_q = 1; model_q <= 2; ++model_q) {
        CHECK(orbx_init_get_scores(b, k, model_q, nullptr, &nit, &why) == ORBX_OK);
        const bool has = P.n >= 8 && (P.models & model_q);
        CHECK(nit == (has ? P.iterations : 0));
        std::vector<float> sc((size_t)(nit > 0 ? nit : 1));
        CHECK(orbx_init_get_scores(b, k, model_q, sc.data(), &nit, &why) == ORBX_OK);
        if (has) {
            CHECK(orbx_init_get_hypothesis(b, k, model_q, nit - 1, M, Mi, &s, nw ? w.data() : nullptr, &why) == ORBX_OK);
            CHECK(orbx_init_get_hypothesis(b, k, model_q, 0, nullptr, nullptr, nullptr, nullptr, &why) == ORBX_OK);
        }
        CHECK(orbx_init_get_hypothesis(b, k, model_q, nit, M, Mi, &s, nullptr, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_init_get_hypothesis(b, k, model_q, -1, M, Mi, &s, nullptr, &why) == ORBX_BAD_ARGUMENT);
    }
    CHECK(orbx_init_get_scores(b, k, 3, nullptr, &nit, &why) == ORBX_BAD_ARGUMENT);
    if (itH >= 0) CHECK(SH > 0.0f && itH < P.iterations);
    if (itF >= 0) CHECK(SF > 0.0f && itF < P.iterations);
    CHECK(model == ORBX_INIT_NONE ? (itH < 0 && itF < 0) : (model == ORBX_INIT_H ? itH >= 0 : itF >= 0));
    return model;
}

int main() {
    const int sizes[] = {8, 9, 63, 64, 65, 129, 257};
    std::vector<Scene> scenes(7);
    std::vector<orbx_init_problem> probs;
    for (int i = 0; i < 7; ++i) {
        make(scenes[i], sizes[i], i == 0 ? 1 : i == 5 ? 60 : 9 + i, 1 + i % 3);
        probs.push_back(scenes[i].P);
    }
    Scene few, empty;                                              // n < 8: launches nothing, its sets are not read
    make(few, 7, 3, 3);
    few.P.sets = nullptr;
    probs.push_back(few.P);
    make(empty, 0, 2, 3, 0, 0);                                    // no keypoints at all: Normalize divides 0 by 0
    empty.P.keys1 = empty.P.keys2 = nullptr; empty.P.matches = nullptr; empty.P.sets = nullptr;
    probs.push_back(empty.P);
    orbx_init_batch *b = run(probs);
    if (b) {
        const char *why = "";
        for (int k = 0; k < 9; ++k) {
            const int32_t model = read_all(b, k, probs[k]);
            if (k == 5) CHECK(model == ORBX_INIT_H);              // 129 matches on a plane, both models
            if (k >= 7) CHECK(model == ORBX_INIT_NONE);
        }
        float T[9];
        CHECK(orbx_init_get_normalization(b, 9, T, T, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_init_get_normalization(b, -1, T, T, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_init_get_normalization(nullptr, 0, T, T, &why) == ORBX_BAD_ARGUMENT);
        delete b;
    }
    // rejections
    {
        Scene s; make(s, 12, 4, 3);
        std::vector<orbx_init_problem> one(1, s.P);
        one[0].n = -1; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].n1 = -1; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].n2 = -1; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].keys1 = nullptr; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].keys2 = nullptr; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].matches = nullptr; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].sets = nullptr; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].iterations = 0; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].models = 4; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        const float sig[] = {0.0f, -1.0f, INFINITY, NAN};
        for (float v : sig) { one[0].sigma = v; run(one, ORBX_BAD_ARGUMENT); }
        one[0] = s.P;
        s.matches[6] = s.P.n1; run(one, ORBX_BAD_ARGUMENT);
        s.matches[6] = 0; s.matches[7] = -1; run(one, ORBX_BAD_ARGUMENT);
        s.matches[7] = s.P.n2; run(one, ORBX_BAD_ARGUMENT);
        s.matches[7] = 3;
        s.sets[13] = 12; run(one, ORBX_BAD_ARGUMENT);
        s.sets[13] = -1; run(one, ORBX_BAD_ARGUMENT);
        s.sets[13] = s.sets[8]; run(one, ORBX_BAD_ARGUMENT);
        OrbxInitPlan plan; const char *why = "";
        CHECK(orbx_init_plan(-1, one.data(), plan, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_init_plan(1, nullptr, plan, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_init_plan(0, nullptr, plan, &why) == ORBX_OK && plan.nlaunch == 0);
    }
    // non-finite and degenerate input runs the same code
    {
        const float poison[] = {INFINITY, NAN, 1e30f, 0.0f};
        for (float v : poison) {
            Scene s; make(s, 70, 6, 3);
            s.k1[2 * (size_t)s.matches[2 * s.sets[0]]] = v;       // a drawn keypoint of frame 1
            s.k2[2 * (size_t)s.matches[2 * s.sets[9] + 1] + 1] = v;
            std::vector<orbx_init_problem> one(1, s.P);
            orbx_init_batch *pb = run(one);
            if (pb) { read_all(pb, 0, one[0]); delete pb; }
        }
        Scene dup; make(dup, 40, 5, 3);                             // the eight matches of set 0 are one point; set 1 is collinear
        for (int c = 0; c < 8; ++c) {
            dup.sets[c] = c; dup.sets[8 + c] = 8 + c;
            dup.k1[2 * (size_t)dup.matches[2 * c]] = 100.0f; dup.k1[2 * (size_t)dup.matches[2 * c] + 1] = 50.0f;
            dup.k2[2 * c] = 120.0f; dup.k2[2 * c + 1] = 60.0f;
            dup.k1[2 * (size_t)dup.matches[2 * (8 + c)]] = 100.0f + 10.0f * c; dup.k1[2 * (size_t)dup.matches[2 * (8 + c)] + 1] = 50.0f + 5.0f * c;
            dup.k2[2 * (8 + c)] = 130.0f + 10.0f * c; dup.k2[2 * (8 + c) + 1] = 70.0f + 5.0f * c;
        }
        std::vector<orbx_init_problem> one(1, dup.P);
        orbx_init_batch *pb = run(one);
        if (pb) {
            int32_t itH = 0;
            const char *why = "";
            read_all(pb, 0, one[0]);
            CHECK(orbx_init_get_result(pb, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &itH, nullptr, nullptr, nullptr, &why) == ORBX_OK);
            CHECK(itH != 0);                                        // H of eight coinciding points is singular: its inverse is not finite
            CHECK(pb->st[0].hyp[0].bad == 1);
            delete pb;
        }
        Scene same; make(same, 20, 3, 3, 0, 0);                     // every keypoint of frame 2 in one place: meanDev = 0, sX = inf
        for (size_t i = 0; i < same.k2.size(); ++i) same.k2[i] = 7.0f;
        std::vector<orbx_init_problem> two(1, same.P);
        orbx_init_batch *sb = run(two);
        if (sb) { CHECK(read_all(sb, 0, two[0]) == ORBX_INIT_NONE); delete sb; }
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
