// san_sim3search.cpp -- csrc/orbx_sim3search.cpp (validation, packing, the host path, the scatter) as a stand-alone program for
// AddressSanitizer + UndefinedBehaviorSanitizer: tests/test_sim3_search_cpu.py builds it with g++ -fsanitize=address,undefined
// together with that unit and runs it.  Keyframes of 0, 1, 63, 64, 65 and 300 features, a batch of problems sharing KF1, null
// and given "already matched" rows, debug rows on and off, non-finite points, every validation failure.  Prints "<n> failures".
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_sim3search.h"

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { ++failures; printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

struct Kf {
    std::vector<orbx_keypoint> keys;
    std::vector<uint8_t> desc, has, pdesc;
    std::vector<float> pos, dmin, dmax;
    explicit Kf(int n, bool poison = false) {
        for (int i = 0; i < n; ++i) {
            const float u = 20.0f + 9.0f * (float)(i % 60), v = 30.0f + 11.0f * (float)(i / 60), z = 2.0f;
            orbx_keypoint k = {u + 0.5f, v, 31.0f, 0.0f, 1.0f, i % 2, -1};
            keys.push_back(k);
            for (int b = 0; b < 32; ++b) { desc.push_back((uint8_t)(i * 7 + b)); pdesc.push_back((uint8_t)(i * 7 + b + (b == 3))); }
            has.push_back(i % 4 != 3);
            pos.push_back((u - 320.0f) / 256.0f * z); pos.push_back((v - 240.0f) / 256.0f * z); pos.push_back(z);
            const float x = pos[pos.size() - 3], y = pos[pos.size() - 2];
            dmin.push_back(0.5f); dmax.push_back(1.1f * sqrtf(x * x + y * y + z * z));   // level 1: octaves 0 and 1 are in the band
        }
        if (poison && n > 8) {
            pos[3 * 1] = std::numeric_limits<float>::quiet_NaN();
            pos[3 * 2 + 2] = 0.0f;
            pos[3 * 4 + 2] = -1.0f;
            pos[3 * 5] = std::numeric_limits<float>::infinity();
            dmax[6] = std::numeric_limits<float>::infinity();
            dmin[8] = std::numeric_limits<float>::quiet_NaN();
        }
    }
    orbx_sim3_search_keyframe view() const {
        orbx_sim3_search_keyframe K = {};
        K.n = (int)keys.size();
        for (int i = 0; i < 4; ++i) K.Tcw[5 * i] = 1.0f;
        if (K.n) {
            K.keys_un = keys.data(); K.desc = desc.data(); K.has_point = has.data(); K.world_pos = pos.data();
            K.min_distance = dmin.data(); K.max_distance = dmax.data(); K.point_desc = pdesc.data();
        }
        return K;
    }
};

static const float CAM[4] = {256.0f, 256.0f, 320.0f, 240.0f}, BND[4] = {0.0f, 640.0f, 0.0f, 480.0f};

struct Out {
    std::vector<std::vector<int32_t>> m, b1, b2, l1, l2;
    std::vector<std::vector<uint8_t>> s1, s2;
    std::vector<std::vector<float>> u1, u2;
    std::vector<int32_t *> mp, b1p, b2p, l1p, l2p;
    std::vector<uint8_t *> s1p, s2p;
    std::vector<float *> u1p, u2p;
    std::vector<int> nf;
    orbx_sim3_search_debug dbg;
};

static orbx_status run(const std::vector<orbx_sim3_search_keyframe> &K, const std::vector<orbx_sim3_search_problem> &P, bool debug,
                       int fma, Out &o, int *total = nullptr) {
    const int np = (int)P.size();
    o = Out();
    o.nf.assign((size_t)np + 1, -9);
    for (int k = 0; k < np; ++k) {
        const bool ok = P[k].kf1 >= 0 && P[k].kf1 < (int)K.size() && P[k].kf2 >= 0 && P[k].kf2 < (int)K.size();
        const size_t n1 = ok && K[P[k].kf1].n > 0 ? (size_t)K[P[k].kf1].n : 0, n2 = ok && K[P[k].kf2].n > 0 ? (size_t)K[P[k].kf2].n : 0;
        o.m.emplace_back(n1, -5); o.b1.emplace_back(n1, -5); o.b2.emplace_back(n2, -5); o.l1.emplace_back(n1, -5); o.l2.emplace_back(n2, -5);
        o.s1.emplace_back(n1, 0xee); o.s2.emplace_back(n2, 0xee); o.u1.emplace_back(2 * n1, -7.0f); o.u2.emplace_back(2 * n2, -7.0f);
    }
    for (int k = 0; k < np; ++k) {                                  // exact-size rows: a write past one is caught
        o.mp.push_back(o.m[k].data()); o.b1p.push_back(o.b1[k].data()); o.b2p.push_back(o.b2[k].data());
        o.l1p.push_back(o.l1[k].data()); o.l2p.push_back(o.l2[k].data()); o.s1p.push_back(o.s1[k].data()); o.s2p.push_back(o.s2[k].data());
        o.u1p.push_back(o.u1[k].data()); o.u2p.push_back(o.u2[k].data());
    }
    o.dbg = {o.s1p.data(), o.s2p.data(), o.b1p.data(), o.b2p.data(), o.l1p.data(), o.l2p.data(), o.u1p.data(), o.u2p.data()};
    OrbxSim3sPlan plan;
    const char *why = "";
    const orbx_status st = orbx_sim3s_plan((int)K.size(), K.data(), np, P.data(), CAM, BND, 8, o.mp.data(), o.nf.data(), plan, &why);
    if (st != ORBX_OK) return st;
    float thr[ORBX_PS_LEVELS], scale[ORBX_PS_LEVELS];
    orbx_predict_scale_build(1.2f, 8, thr);
    float s = 1.0f;
    for (int l = 0; l < ORBX_PS_LEVELS; ++l) { scale[l] = s; s *= 1.2f; }
    OrbxSim3sCam cam;
    OrbxSim3sGrid grid;
    orbx_sim3s_camera(CAM, BND, fma, 8, thr, scale, cam, grid);
    std::vector<uint8_t> in(plan.in_bytes), out(plan.out_bytes);     // exact sizes: a write past the layout is caught
    orbx_sim3s_pack(K.data(), P.data(), plan, in.data());
    orbx_sim3s_host_run(plan, cam, grid, in.data(), out.data());
    orbx_sim3s_unpack(plan, in.data(), out.data(), o.mp.data(), o.nf.data(), debug ? &o.dbg : nullptr);
    int t = 0;
    for (int k = 0; k < np; ++k) {
        int c = 0;
        for (int32_t v : o.m[k]) { EXPECT(v >= -1 && v < K[P[k].kf2].n); c += v >= 0; }
        EXPECT(c == o.nf[k]);
        t += c;
        if (debug)
            for (size_t i = 0; i < o.s1[k].size(); ++i) EXPECT(o.s1[k][i] <= ORBX_SIM3S_MATCH && (o.b1[k][i] >= 0) == (o.s1[k][i] == ORBX_SIM3S_MATCH));
        else
            for (uint8_t v : o.s1[k]) EXPECT(v == 0xee);
    }
    EXPECT(o.nf[(size_t)np] == -9);
    if (total) *total = t;
    return ORBX_OK;
}

static orbx_sim3_search_problem prob(int kf1, int kf2, float s12 = 1.0f, const uint8_t *m1 = nullptr, const uint8_t *m2 = nullptr) {
    orbx_sim3_search_problem P = {};
    P.kf1 = kf1; P.kf2 = kf2; P.s12 = s12; P.th = 7.5f;
    P.R12[0] = P.R12[4] = P.R12[8] = 1.0f;
    P.matched1 = m1; P.matched2 = m2;
    return P;
}

// the predict-scale table lives in orbx_track_pack.cpp in the library; this program carries the few lines it needs
void orbx_predict_scale_build(float scale_factor, int nlevels, float *thr) {
    const float lsf = logf(scale_factor);
    thr[0] = 0.0f;
    for (int k = 1; k < ORBX_PS_LEVELS; ++k) {
        thr[k] = std::numeric_limits<float>::infinity();
        if (k >= nlevels) continue;
        float r = (float)pow((double)scale_factor, (double)(k - 1));
        while ((int)ceilf(logf(r) / lsf) < k) r = nextafterf(r, std::numeric_limits<float>::infinity());
        thr[k] = r;
    }
}

int main() {
    const int sizes[] = {65, 0, 1, 63, 64, 300};
    std::vector<Kf> kf;
    for (int n : sizes) kf.emplace_back(n, n == 300);
    std::vector<orbx_sim3_search_keyframe> K;
    for (const Kf &k : kf) K.push_back(k.view());
    Out o;
    int total = 0;
    // the shared-KF1 batch: every keyframe against KF 0, KF 0 against itself, both fp modes, debug rows on and off
    std::vector<uint8_t> m1(65, 0), m2(300, 0), all(65, 1);
    m1[3] = m1[10] = 1; m2[7] = 1;
    std::vector<orbx_sim3_search_problem> P;
    for (int k = 0; k < (int)K.size(); ++k) P.push_back(prob(0, k));
    P.push_back(prob(0, 5, 1.0f, m1.data(), m2.data()));
    P.push_back(prob(0, 4, 1.0f, all.data(), nullptr));
    P.push_back(prob(5, 0, 0.5f));
    for (int fma = 0; fma < 2; ++fma)
        for (int debug = 0; debug < 2; ++debug) {
            EXPECT(run(K, P, debug != 0, fma, o, &total) == ORBX_OK);
            EXPECT(total > 60);
            EXPECT(o.nf[0] > 30 && o.nf[1] == 0 && o.nf[7] == 0);
            EXPECT(o.m[6][3] == -1 && o.m[6][10] == -1);
        }
    // a keyframe at a time against itself: sizes around 64 and the empty one
    for (int k = 0; k < (int)K.size(); ++k) {
        std::vector<orbx_sim3_search_problem> one(1, prob(k, k));
        EXPECT(run(K, one, true, 1, o, &total) == ORBX_OK);
        EXPECT((sizes[k] == 0) == (total == 0) || sizes[k] == 1);
    }
    // no problem, no keyframe
    EXPECT(run(K, {}, false, 1, o) == ORBX_OK);
    EXPECT(run({}, {}, false, 1, o) == ORBX_OK);
    // validation
    {
        OrbxSim3sPlan plan;
        const char *why = "";
        std::vector<int32_t> row(65);
        int32_t *rows[1] = {row.data()};
        int nf[1];
        std::vector<orbx_sim3_search_problem> one(1, prob(0, 4));
        auto plan_of = [&](const std::vector<orbx_sim3_search_keyframe> &kk, int nk, int np, const float *cam, const float *bnd, int nlevels,
                           int32_t *const *r, int *f) {
            return orbx_sim3s_plan(nk, nk ? kk.data() : nullptr, np, one.data(), cam, bnd, nlevels, r, f, plan, &why);
        };
        EXPECT(plan_of(K, 6, 1, CAM, BND, 8, rows, nf) == ORBX_OK);
        EXPECT(plan_of(K, -1, 1, CAM, BND, 8, rows, nf) == ORBX_BAD_ARGUMENT);
        EXPECT(plan_of(K, 6, -1, CAM, BND, 8, rows, nf) == ORBX_BAD_ARGUMENT);
        EXPECT(plan_of(K, 6, 1, nullptr, BND, 8, rows, nf) == ORBX_BAD_ARGUMENT);
        EXPECT(plan_of(K, 6, 1, CAM, nullptr, 8, rows, nf) == ORBX_BAD_ARGUMENT);
        EXPECT(plan_of(K, 6, 1, CAM, BND, 8, nullptr, nf) == ORBX_BAD_ARGUMENT);
        EXPECT(plan_of(K, 6, 1, CAM, BND, 8, rows, nullptr) == ORBX_BAD_ARGUMENT);
        EXPECT(plan_of(K, 6, 1, CAM, BND, 1, rows, nf) == ORBX_BAD_ARGUMENT);      // octave 1 outside one level
        EXPECT(plan_of(K, 4, 1, CAM, BND, 8, rows, nf) == ORBX_BAD_ARGUMENT);      // kf2 = 4 outside a pool of 4
        const float flat[4] = {0.0f, 0.0f, 0.0f, 480.0f};
        EXPECT(plan_of(K, 6, 1, CAM, flat, 8, rows, nf) == ORBX_BAD_ARGUMENT);
        int32_t *norow[1] = {nullptr};
        EXPECT(plan_of(K, 6, 1, CAM, BND, 8, norow, nf) == ORBX_BAD_ARGUMENT);
        std::vector<orbx_sim3_search_keyframe> bad = K;
        bad[4].point_desc = nullptr;
        EXPECT(plan_of(bad, 6, 1, CAM, BND, 8, rows, nf) == ORBX_BAD_ARGUMENT);
        bad = K; bad[2].n = -1;
        EXPECT(plan_of(bad, 6, 1, CAM, BND, 8, rows, nf) == ORBX_BAD_ARGUMENT);
        bad = K; bad[2].n = 65536;
        EXPECT(plan_of(bad, 6, 1, CAM, BND, 8, rows, nf) == ORBX_UNSUPPORTED);
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
