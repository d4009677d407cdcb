// tests/san_recon.cpp -- a stand-alone program around csrc/orbx_recon.cpp (validation, packing, the host path, acos and the
// accept / reject arithmetic, the result object; HIP-free), built by tests/test_recon_cpu.py with g++ -fsanitize=address,undefined:
// sizes around the ballot words, both models, every rejection, problems that launch nothing, non-finite input, and the
// continuation of a RANSAC batch (orbx_recon_problems_from, orbx_recon_batch_new_fused's bookkeeping).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_recon.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static uint64_t g_state = 7;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(g_state >> 33); }
static double uni(double a, double b) { return a + (b - a) * (rnd() / 2147483648.0); }

struct Scene {
    std::vector<float> k1, k2;
    std::vector<int32_t> matches;
    std::vector<uint8_t> inl;
    orbx_recon_problem P;
};

// n points in front of two cameras (a rotation about y and a translation; on a plane for H), every fifth match displaced by 40 px
// and left out of the mask; match i pairs keypoint n - 1 - i of frame 1 with keypoint i of frame 2
static void make(Scene &S, int n, int model) {
    const double fx = 500, fy = 500, cx = 320, cy = 240, a = 0.1, c = cos(a), s = sin(a), t[3] = {0.5, 0.05, 0.1};
    const double nrm[3] = {-0.3, 0.2, 1.0}, d = 6.0;
    S.k1.assign((size_t)n * 2, 0.0f); S.k2.assign((size_t)n * 2, 0.0f); S.matches.assign((size_t)n * 2, 0); S.inl.assign((size_t)n, 1);
    for (int i = 0; i < n; ++i) {
        const int f = n - 1 - i;
        double X = uni(-2.5, 2.5), Y = uni(-1.8, 1.8), Z = uni(4, 9);
        if (model == ORBX_INIT_H) Z = d + 0.3 * X - 0.2 * Y;
        const double X2 = c * X + s * Z + t[0], Y2 = Y + t[1], Z2 = -s * X + c * Z + t[2];
        S.k1[2 * f] = (float)(fx * X / Z + cx); S.k1[2 * f + 1] = (float)(fy * Y / Z + cy);
        S.k2[2 * i] = (float)(fx * X2 / Z2 + cx + (i % 5 == 4 ? 40.0 : 0.0)); S.k2[2 * i + 1] = (float)(fy * Y2 / Z2 + cy);
        S.matches[2 * i] = f; S.matches[2 * i + 1] = i;
        if (i % 5 == 4) S.inl[i] = 0;
    }
    const double R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    double G[9];                                                    // R + t nrm^T / d, or [t]x R
    const double tx[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            G[3 * i + j] = model == ORBX_INIT_H ? R[3 * i + j] + t[i] * nrm[j] / d
                                                : tx[3 * i] * R[j] + tx[3 * i + 1] * R[3 + j] + tx[3 * i + 2] * R[6 + j];
    const double Km[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1}, Ki[9] = {1 / fx, 0, -cx / fx, 0, 1 / fy, -cy / fy, 0, 0, 1};
    double T[9], M[9];
    for (int i = 0; i < 3; ++i)                                    // H: K G Kinv; F: Kinv^T G Kinv
        for (int j = 0; j < 3; ++j) {
            T[3 * i + j] = 0;
            for (int k = 0; k < 3; ++k) T[3 * i + j] += (model == ORBX_INIT_H ? Km[3 * i + k] : Ki[3 * k + i]) * G[3 * k + j];
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            M[3 * i + j] = 0;
            for (int k = 0; k < 3; ++k) M[3 * i + j] += T[3 * i + k] * Ki[3 * k + j];
        }
    memset(&S.P, 0, sizeof(S.P));
    S.P.n1 = S.P.n2 = S.P.n = n;
    S.P.keys1 = n ? S.k1.data() : nullptr; S.P.keys2 = n ? S.k2.data() : nullptr;
    S.P.matches = n ? S.matches.data() : nullptr; S.P.inliers = n ? S.inl.data() : nullptr;
    S.P.model = model;
    for (int i = 0; i < 9; ++i) S.P.M[i] = (float)M[i];
    S.P.K[0] = 500; S.P.K[1] = 500; S.P.K[2] = 320; S.P.K[3] = 240;
    S.P.sigma = 1.0f; S.P.min_parallax = 1.0f; S.P.min_triangulated = 50;
}

static orbx_recon_batch *run(const std::vector<orbx_recon_problem> &probs, orbx_status want = ORBX_OK) {
    OrbxReconPlan plan;
    const char *why = "";
    const orbx_status st = orbx_recon_plan((int)probs.size(), probs.data(), plan, &why);
    CHECK(st == want);
    if (st != ORBX_OK) return nullptr;
    orbx_recon_batch *b = orbx_recon_batch_new(probs.data(), plan);
    if (plan.nlaunch > 0) {
        std::vector<uint8_t> in(plan.in_bytes), out(plan.out_bytes);
        orbx_recon_pack(probs.data(), plan, in.data());
        orbx_recon_host_run(plan, in.data(), out.data());
        orbx_recon_batch_take(b, plan, out.data());
    }
    return b;
}

// every accessor of problem k into buffers of exactly the documented sizes; returns ok
static int32_t read_all(orbx_recon_batch *b, int k, const orbx_recon_problem &P) {
    const char *why = "";
    const size_t n = (size_t)P.n;
    std::vector<uint8_t> st(n);
    std::vector<float> pts(3 * n);
    float R[9], t[3], nv[3], c, par;
    int32_t ok, chosen, N, nGood, valid;
    CHECK(orbx_recon_get_result(b, k, &ok, R, t, &chosen, n ? st.data() : nullptr, n ? pts.data() : nullptr, &N, &why) == ORBX_OK);
    CHECK(orbx_recon_get_result(b, k, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &why) == ORBX_OK);
    const int nh = P.model == ORBX_INIT_H ? 8 : 4;
    for (int i = 0; i < nh; ++i) {
        CHECK(orbx_recon_get_hypothesis(b, k, i, R, t, nv, &nGood, &c, &par, &valid, &why) == ORBX_OK);
        CHECK(nGood >= 0 && nGood <= N);
    }
    CHECK(orbx_recon_get_hypothesis(b, k, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &why) == ORBX_OK);
    CHECK(orbx_recon_get_hypothesis(b, k, nh, R, t, nv, &nGood, &c, &par, &valid, &why) == ORBX_BAD_ARGUMENT);
    CHECK(orbx_recon_get_hypothesis(b, k, -1, R, t, nv, &nGood, &c, &par, &valid, &why) == ORBX_BAD_ARGUMENT);
    CHECK(chosen >= -1 && chosen < nh && (!ok || chosen >= 0));
    return ok;
}

int main() {
    const int sizes[] = {1, 8, 63, 64, 65, 129, 257};
    std::vector<Scene> scenes(14);
    std::vector<orbx_recon_problem> probs;
    for (int i = 0; i < 14; ++i) {
        make(scenes[i], sizes[i % 7], i < 7 ? ORBX_INIT_F : ORBX_INIT_H);
        probs.push_back(scenes[i].P);
    }
    Scene none, empty;                                             // an all-false mask and no match at all: nothing launches
    make(none, 20, ORBX_INIT_F);
    std::fill(none.inl.begin(), none.inl.end(), 0);
    probs.push_back(none.P);
    make(empty, 0, ORBX_INIT_H);
    probs.push_back(empty.P);
    orbx_recon_batch *b = run(probs);
    if (b) {
        const char *why = "";
        for (int k = 0; k < 16; ++k) {
            const int32_t ok = read_all(b, k, probs[k]);
            if (k == 5 || k == 6) CHECK(ok == 1);                  // 129 and 257 matches of a general scene through F
            if (k >= 14) CHECK(ok == 0 && b->st[k].chosen == -1);
        }
        CHECK(orbx_recon_get_result(b, 16, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_recon_get_result(b, -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_recon_get_result(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &why) == ORBX_BAD_ARGUMENT);
        delete b;
    }
    // rejections
    {
        Scene s; make(s, 12, ORBX_INIT_F);
        std::vector<orbx_recon_problem> one(1, s.P);
        one[0].n = -1; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].n1 = -1; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].n2 = -1; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].keys1 = nullptr; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].keys2 = nullptr; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].matches = nullptr; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].inliers = nullptr; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].model = 0; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].model = 3; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        const float bad[] = {0.0f, -1.0f, INFINITY, NAN};
        for (float v : bad) { one[0].sigma = v; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P; }
        for (float v : bad) { one[0].K[0] = v; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P; }
        for (float v : bad) { one[0].K[1] = v; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P; }
        one[0].K[2] = NAN; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].K[3] = INFINITY; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        one[0].min_parallax = NAN; run(one, ORBX_BAD_ARGUMENT); one[0] = s.P;
        s.matches[6] = s.P.n1; run(one, ORBX_BAD_ARGUMENT);
        s.matches[6] = 0; s.matches[7] = -1; run(one, ORBX_BAD_ARGUMENT);
        s.matches[7] = s.P.n2; run(one, ORBX_BAD_ARGUMENT);
        s.matches[7] = 3;
        OrbxReconPlan plan; const char *why = "";
        CHECK(orbx_recon_plan(-1, one.data(), plan, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_recon_plan(1, nullptr, plan, &why) == ORBX_BAD_ARGUMENT);
        CHECK(orbx_recon_plan(0, nullptr, plan, &why) == ORBX_OK && plan.nlaunch == 0);
    }
    // non-finite and degenerate input runs the same code
    {
        const float poison[] = {INFINITY, NAN, 1e30f, 0.0f};
        for (int model = ORBX_INIT_H; model <= ORBX_INIT_F; ++model)
            for (float v : poison) {
                Scene s; make(s, 70, model);
                s.k1[10] = v; s.k2[31] = v;
                std::vector<orbx_recon_problem> one(1, s.P);
                orbx_recon_batch *pb = run(one);
                if (pb) { read_all(pb, 0, one[0]); delete pb; }
                one[0].M[4] = v;                                    // and a matrix that is not finite, or singular
                pb = run(one);
                if (pb) { read_all(pb, 0, one[0]); delete pb; }
                for (int i = 0; i < 9; ++i) one[0].M[i] = v;
                pb = run(one);
                if (pb) { read_all(pb, 0, one[0]); delete pb; }
            }
        Scene same; make(same, 30, ORBX_INIT_F);                    // every keypoint of frame 2 in one place; a repeated first index
        for (size_t i = 0; i < same.k2.size(); ++i) same.k2[i] = 7.0f;
        same.matches[2] = same.matches[0];
        std::vector<orbx_recon_problem> one(1, same.P);
        orbx_recon_batch *pb = run(one);
        if (pb) { CHECK(read_all(pb, 0, one[0]) == 0); delete pb; }
    }
    // the continuation of a RANSAC batch: a winning H, a winning F, no model, and a problem that launched nothing
    {
        Scene s; make(s, 40, ORBX_INIT_F);
        orbx_init_problem ip[4];
        orbx_init_camera cam[4];
        orbx_init_batch ib;
        ib.st.resize(4);
        for (int k = 0; k < 4; ++k) {
            memset(&ip[k], 0, sizeof(ip[k]));
            ip[k].n1 = ip[k].n2 = ip[k].n = 40; ip[k].keys1 = s.k1.data(); ip[k].keys2 = s.k2.data(); ip[k].matches = s.matches.data();
            ip[k].sigma = 1.0f; ip[k].iterations = 2; ip[k].models = 3;
            memcpy(cam[k].K, s.P.K, sizeof(cam[k].K)); cam[k].min_parallax = 1.0f; cam[k].min_triangulated = 50;
            OrbxInitResult &R = ib.st[k];
            R.n = 40; R.iterations = 2; R.nwords = 1; R.models = 3; R.launches = k != 3;
            R.hyp.resize(4); R.masks.assign(4, 0); R.scores.assign(4, 0.0f);
            for (int l = 0; l < 4; ++l) { memcpy(R.hyp[l].M, s.P.M, sizeof(s.P.M)); R.masks[l] = 0xff0ffffffull >> l; }
            R.itH = k == 0 ? 1 : -1; R.itF = k == 1 ? 0 : -1;
            R.model = k == 0 ? ORBX_INIT_H : k == 1 ? ORBX_INIT_F : ORBX_INIT_NONE;
        }
        std::vector<orbx_recon_problem> rp;
        std::vector<std::vector<uint8_t>> store;
        orbx_recon_problems_from(ip, cam, &ib, rp, store);
        CHECK(rp.size() == 4 && rp[0].model == ORBX_INIT_H && rp[1].model == ORBX_INIT_F && rp[2].model == ORBX_INIT_F);
        orbx_recon_batch *pb = run(rp);
        orbx_recon_batch *fb = orbx_recon_batch_new_fused(cam, &ib);
        if (pb) {
            for (int k = 0; k < 4; ++k) {
                read_all(pb, k, rp[k]);
                CHECK(fb->st[k].N == pb->st[k].N && fb->st[k].launches == pb->st[k].launches && fb->st[k].nhyp == pb->st[k].nhyp);
                CHECK(fb->st[k].slot == (k != 3));
            }
            CHECK(pb->st[0].N == 31 && pb->st[1].N == 30 && pb->st[2].N == 0 && pb->st[3].N == 0);
            delete pb;
        }
        delete fb;
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
