// san_localba.cpp -- stand-alone driver of csrc/orbx_localba.cpp (the HIP-free validation, packing with the derived index lists,
// host path and scatter of the batched Optimizer::LocalBundleAdjustment) for AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_localba_cpu.py builds and runs it).  Every caller array is an exactly sized heap block, so that a read or write
// past one is a report; the staging blocks are exactly plan.in_bytes, plan.work_bytes and plan.out_bytes long.  Two scenes run
// through the host path in one batch (mixed edges with a locally fixed keyframe; monocular with no fixed keyframe and one
// round), then the classification alone, then every rejection, then a scene with a NaN point.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined tools/san_localba.cpp \
//       orb_slam2_detailed_comments_amd/csrc/orbx_localba.cpp -o san_localba && ./san_localba
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_localba.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static std::mt19937 rng(31);
static float uni(float lo, float hi) { return lo + (hi - lo) * (float)(rng() >> 8) / 16777216.0f; }

struct Scene {
    std::vector<float> Tcw, world, obs, w, Tout, wout;
    std::vector<uint8_t> lf, erase;
    std::vector<int32_t> begin, kf;
    orbx_localba_problem P;
};
// keyframes along x looking down z (no rotation), points 3 to 8 metres ahead, every point seen by every second keyframe at least
static void make(Scene &S, int nlocal, int nfixed, int npoints, bool stereo, int fixed_local, int second_round) {
    const int nkf = nlocal + nfixed;
    S.Tcw.assign(16 * (size_t)nkf, 0.f);
    for (int k = 0; k < nkf; ++k) {
        float *T = &S.Tcw[16 * (size_t)k];
        T[0] = T[5] = T[10] = T[15] = 1.f;
        T[3] = -0.3f * (float)k + (k < nlocal && k != fixed_local ? uni(-0.02f, 0.02f) : 0.f);
    }
    S.lf.assign((size_t)nlocal, 0);
    if (fixed_local >= 0) S.lf[(size_t)fixed_local] = 1;
    S.world.resize(3 * (size_t)npoints);
    S.begin.assign(1, 0);
    S.kf.clear(); S.obs.clear(); S.w.clear();
    for (int p = 0; p < npoints; ++p) {
        const float X = uni(-1.f, 2.f), Y = uni(-1.f, 1.f), Z = uni(3.f, 8.f);
        S.world[3 * (size_t)p] = X + uni(-0.03f, 0.03f); S.world[3 * (size_t)p + 1] = Y + uni(-0.03f, 0.03f); S.world[3 * (size_t)p + 2] = Z + uni(-0.03f, 0.03f);
        for (int k = nkf - 1; k >= 0; --k) {                    // (descending: the caller's order is no particular one)
            if ((k + p) % 2 && nkf > 2) continue;
            const float x = X - 0.3f * (float)k, gross = rng() % 10 == 0 ? 30.f : 0.f;
            const float u = 100.f * x / Z + 80.f + uni(-0.5f, 0.5f) + gross, v = 100.f * Y / Z + 60.f + uni(-0.5f, 0.5f);
            S.kf.push_back(k);
            S.obs.push_back(u); S.obs.push_back(v); S.obs.push_back(stereo && rng() % 2 ? u - 10.f / Z : -1.f);
            S.w.push_back(1.0f / (float)std::pow(1.44, (double)(rng() % 8)));
        }
        S.begin.push_back((int32_t)S.kf.size());
    }
    S.Tout.assign(16 * (size_t)nlocal, 7.5f); S.wout.assign(3 * (size_t)npoints, 7.5f); S.erase.assign(S.kf.size(), 9);
    orbx_localba_problem &P = S.P;
    memset(&P, 0, sizeof(P));
    P.nlocal = nlocal; P.nfixed = nfixed; P.npoints = npoints; P.second_round = second_round;
    P.Tcw = S.Tcw.data(); P.local_fixed = S.lf.data(); P.world = S.world.data();
    const float cam[4] = {100.f, 100.f, 80.f, 60.f};
    memcpy(P.camera, cam, sizeof(cam));
    P.bf = 10.f;
    P.obs_begin = S.begin.data(); P.obs_kf = S.kf.data(); P.obs = S.obs.data(); P.inv_sigma2 = S.w.data();
    P.Tcw_out = S.Tout.data(); P.world_out = S.wout.data(); P.erase = S.erase.data();
}

static orbx_status call(int n, const orbx_localba_problem *probs, const orbx_localba_debug *dbg, orbx_localba_result *res) {
    OrbxLbaPlan plan;
    std::vector<DLbaProb> dp;
    const char *why = "";
    const orbx_status st = orbx_localba_plan(n, probs, res, dbg, dbg != nullptr, plan, dp, &why);
    if (st != ORBX_OK || n == 0) return st;
    uint8_t *in = (uint8_t *)malloc(plan.in_bytes), *work = (uint8_t *)malloc(plan.work_bytes), *out = (uint8_t *)malloc(plan.out_bytes);
    memset(work, 0xCD, plan.work_bytes);                       // the device workspace is not cleared either
    orbx_localba_pack(probs, dbg, plan, dp, in);
    orbx_localba_host_run(plan, in, work, out);
    orbx_localba_unpack(probs, dp, out, dbg != nullptr, res);
    free(in); free(work); free(out);
    return ORBX_OK;
}

int main() {
    Scene A, B;
    make(A, 4, 2, 70, true, 1, 1);
    make(B, 3, 0, 65, false, -1, 0);
    orbx_localba_problem probs[2] = {A.P, B.P};
    orbx_localba_result res[2];
    CHECK(call(2, probs, nullptr, res) == ORBX_OK);
    CHECK(res[0].iters[0] >= 1 && res[0].iters[0] <= 5 && res[0].iters[1] >= 1 && res[0].iters[1] <= 10);
    CHECK(res[1].iters[0] >= 1 && res[1].iters[1] == 0 && res[1].nflagged == 0);
    CHECK(res[0].chi2[1] <= res[0].chi2[0] && res[0].nerase > 0);
    int ne = 0;
    for (uint8_t e : A.erase) { CHECK(e <= 1); ne += e; }
    CHECK(ne == res[0].nerase);
    for (float v : A.Tout) CHECK(v != 7.5f);
    for (float v : B.wout) CHECK(v != 7.5f);
    // the classification alone: est = the optimised estimates, last = the start
    std::vector<float> Te(A.Tcw), we(A.wout);
    memcpy(Te.data(), A.Tout.data(), A.Tout.size() * sizeof(float));
    orbx_localba_debug D = {Te.data(), we.data(), A.Tcw.data(), A.world.data()};
    CHECK(call(1, &A.P, &D, res) == ORBX_OK);
    CHECK(res[0].nerase >= 0);
    // rejections: nothing is written
    Scene C;
    make(C, 2, 1, 10, true, -1, 1);
    orbx_localba_problem bad = C.P;
    bad.nlocal = 129; CHECK(call(1, &bad, nullptr, res) == ORBX_UNSUPPORTED);
    bad = C.P; bad.npoints = -1; CHECK(call(1, &bad, nullptr, res) == ORBX_BAD_ARGUMENT);
    bad = C.P; bad.world = nullptr; CHECK(call(1, &bad, nullptr, res) == ORBX_BAD_ARGUMENT);
    const int32_t k3 = C.kf[3], k1 = C.kf[1];
    C.kf[3] = 3; CHECK(call(1, &C.P, nullptr, res) == ORBX_BAD_ARGUMENT);
    C.kf[3] = k3; C.kf[1] = C.kf[0]; CHECK(C.begin[1] == 2 && call(1, &C.P, nullptr, res) == ORBX_BAD_ARGUMENT);   // one keyframe twice
    C.kf[1] = k1;
    CHECK(call(-1, &C.P, nullptr, res) == ORBX_BAD_ARGUMENT);
    CHECK(call(0, nullptr, nullptr, nullptr) == ORBX_OK);
    for (float v : C.Tout) CHECK(v == 7.5f);
    for (uint8_t e : C.erase) CHECK(e == 9);
    // outside the contract: a NaN point; the loops are bounded and the stored NaNs canonical
    Scene E;
    make(E, 3, 1, 20, true, -1, 1);
    E.world[4] = NAN;
    CHECK(call(1, &E.P, nullptr, res) == ORBX_OK);
    CHECK(res[0].iters[0] <= 5 && res[0].iters[1] <= 10);
    for (float v : E.wout) { uint32_t b; memcpy(&b, &v, 4); CHECK(v == v || b == 0x7fc00000u); }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
