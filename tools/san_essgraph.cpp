// san_essgraph.cpp -- stand-alone driver of csrc/orbx_essgraph.cpp (the HIP-free validation, elimination order and symbolic
// factorisation, packing, host path and scatter of the batched Optimizer::OptimizeEssentialGraph) for AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_essgraph_cpu.py builds and runs it).  Every caller array is an exactly sized heap block,
// so that a read or write past one is a report; the staging blocks are exactly plan.in_bytes, plan.work_bytes and
// plan.out_bytes long.  Three scenes run through the host path in one batch (a path of 40 with covisibility edges and points;
// a star whose hub has 70 edges, under fix_scale; an 8-cycle with a chord, parallel edges, a vertex without an edge and a
// component without a fixed vertex), then the cap of the device path on a complete graph, then every rejection.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined tools/san_essgraph.cpp \
//       orb_slam2_detailed_comments_amd/csrc/orbx_essgraph.cpp -o san_essgraph && ./san_essgraph
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_essgraph.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static std::mt19937 rng(17);
static double uni(double lo, double hi) { return lo + (hi - lo) * (double)(rng() >> 8) / 16777216.0; }

struct Scene {
    std::vector<double> Scw, nc, Sout;
    std::vector<uint8_t> fixed, has;
    std::vector<int32_t> edges, ref;
    std::vector<float> world, Tout, wout;
    orbx_essgraph_problem P;
};
static void pose(double *S, double ax, double ay, double az, double tx, double ty, double tz, double s) {
    const double th = std::sqrt(ax * ax + ay * ay + az * az), k = th > 0 ? std::sin(th / 2) / th : 0.0;
    S[0] = k * ax; S[1] = k * ay; S[2] = k * az; S[3] = std::cos(th / 2); S[4] = tx; S[5] = ty; S[6] = tz; S[7] = s;
}
static void make(Scene &S, int nv, const std::vector<int32_t> &edges, int fixed_vertex, int fix_scale, int npoints) {
    S.Scw.resize(8 * (size_t)nv); S.nc.resize(8 * (size_t)nv); S.Sout.assign(8 * (size_t)nv, 7.5);
    S.fixed.assign((size_t)nv, 0); S.has.assign((size_t)nv, 1);
    for (int v = 0; v < nv; ++v) {
        const double a[3] = {uni(-0.5, 0.5), uni(-0.5, 0.5), uni(-0.5, 0.5)}, t[3] = {uni(-3, 3), uni(-3, 3), uni(-3, 3)};
        const double s = fix_scale ? 1.0 : uni(0.8, 1.2);
        pose(&S.nc[8 * (size_t)v], a[0], a[1], a[2], t[0], t[1], t[2], s);
        pose(&S.Scw[8 * (size_t)v], a[0] + uni(-0.01, 0.01), a[1] + uni(-0.01, 0.01), a[2], t[0] + uni(-0.03, 0.03), t[1], t[2],
             fix_scale ? 1.0 : s * uni(0.99, 1.01));
    }
    if (fixed_vertex >= 0) { S.fixed[(size_t)fixed_vertex] = 1; memcpy(&S.Scw[8 * (size_t)fixed_vertex], &S.nc[8 * (size_t)fixed_vertex], 64); }
    S.edges = edges;
    S.world.resize(3 * (size_t)npoints); S.ref.resize((size_t)npoints);
    for (int p = 0; p < npoints; ++p) {
        for (int a = 0; a < 3; ++a) S.world[3 * (size_t)p + a] = (float)uni(-4, 4);
        S.ref[(size_t)p] = p % 7 == 3 ? -1 : (int32_t)(rng() % (unsigned)nv);
    }
    S.Tout.assign(16 * (size_t)nv, 7.5f); S.wout.assign(3 * (size_t)npoints, 7.5f);
    memset(&S.P, 0, sizeof(S.P));
    S.P.nvertices = nv; S.P.nedges = (int32_t)(edges.size() / 3); S.P.npoints = npoints; S.P.fix_scale = fix_scale;
    S.P.Scw = S.Scw.data(); S.P.fixed = S.fixed.data(); S.P.non_corrected = S.nc.data(); S.P.has_non_corrected = S.has.data();
    S.P.edges = S.edges.data(); S.P.world = S.world.data(); S.P.ref = S.ref.data();
    S.P.Siw_out = S.Sout.data(); S.P.Tiw_out = S.Tout.data(); S.P.world_out = S.wout.data();
}
static orbx_status run(const orbx_essgraph_problem *P, int n, orbx_essgraph_result *res, bool cap, const char **why) {
    OrbxEgPlan plan;
    const orbx_status st = orbx_eg_plan(n, P, res, cap, plan, why);
    if (st != ORBX_OK || n == 0) return st;
    uint8_t *in = (uint8_t *)malloc(plan.in_bytes), *work = (uint8_t *)malloc(plan.work_bytes), *out = (uint8_t *)malloc(plan.out_bytes);
    memset(in, 0, plan.in_bytes);
    orbx_eg_pack(P, plan, in);
    orbx_eg_host_run(plan, in, work, out);
    orbx_eg_unpack(P, plan, out, res);
    free(in); free(work); free(out);
    return st;
}
static void edge(std::vector<int32_t> &e, int i, int j, int kind) { e.push_back(i); e.push_back(j); e.push_back(kind); }

int main() {
    const char *why = "";
    Scene A, B, Cc;
    std::vector<int32_t> e;
    for (int i = 1; i < 40; ++i) for (int k = 1; k <= 3 && i - k >= 0; ++k) edge(e, i, i - k, 0);
    edge(e, 39, 0, 1);
    make(A, 40, e, 0, 0, 70);
    e.clear();
    for (int i = 1; i <= 70; ++i) edge(e, i, 0, 0);
    make(B, 71, e, 1, 1, 1);
    e.clear();
    edge(e, 1, 0, 0);
    for (int i = 1; i < 8; ++i) edge(e, i + 1, i, 0);
    edge(e, 8, 1, 0); edge(e, 5, 1, 0); edge(e, 5, 1, 1);       // the chord twice: parallel edges
    edge(e, 11, 10, 0); edge(e, 12, 11, 0); edge(e, 12, 10, 1); // a component without a fixed vertex; vertex 9 has no edge
    make(Cc, 13, e, 0, 0, 0);
    orbx_essgraph_problem P[3] = {A.P, B.P, Cc.P};
    orbx_essgraph_result res[3];
    CHECK(run(P, 3, res, true, &why) == ORBX_OK);
    CHECK(res[0].nactive == 39 && res[0].iters >= 1 && res[0].chi2[1] < res[0].chi2[0] && res[0].nfailed == 0);
    CHECK(res[1].nactive == 70 && res[1].nrounds == 2 && res[1].nlblocks == 139);
    for (int v = 0; v < 71; ++v) CHECK(B.Sout[8 * (size_t)v + 7] == 1.0);
    CHECK(res[2].nactive == 11 && res[2].nlblocks > 11 + 11);
    CHECK(memcmp(&Cc.Sout[8 * 9], &Cc.Scw[8 * 9], 64) == 0);
    for (size_t p = 0; p < 70; ++p) if (A.ref[p] < 0) CHECK(memcmp(&A.wout[3 * p], &A.world[3 * p], 12) == 0); else CHECK(A.wout[3 * p] != 7.5f);
    CHECK(run(P, 0, res, true, &why) == ORBX_OK);
    // the cap of the device path: a complete graph on 256 free vertices
    {
        Scene K;
        e.clear();
        for (int i = 0; i < 257; ++i) for (int j = 0; j < i; ++j) edge(e, i, j, 0);
        make(K, 257, e, 0, 0, 0);
        CHECK(run(&K.P, 1, res, true, &why) == ORBX_CAPACITY);
        CHECK(K.Sout[0] == 7.5);
    }
    // rejections: nothing is written
    {
        Scene R;
        e.clear();
        for (int i = 1; i < 6; ++i) edge(e, i, i - 1, 0);
        make(R, 6, e, 0, 0, 4);
        orbx_essgraph_problem Q = R.P;
        CHECK(run(&Q, -1, res, true, &why) == ORBX_BAD_ARGUMENT);
        CHECK(run(nullptr, 1, res, true, &why) == ORBX_BAD_ARGUMENT);
        CHECK(run(&Q, 1, nullptr, true, &why) == ORBX_BAD_ARGUMENT);
        Q = R.P; Q.nvertices = -1; CHECK(run(&Q, 1, res, true, &why) == ORBX_BAD_ARGUMENT);
        Q = R.P; Q.Scw = nullptr; CHECK(run(&Q, 1, res, true, &why) == ORBX_BAD_ARGUMENT);
        Q = R.P; Q.has_non_corrected = nullptr; CHECK(run(&Q, 1, res, true, &why) == ORBX_BAD_ARGUMENT);
        Q = R.P; Q.edges = nullptr; CHECK(run(&Q, 1, res, true, &why) == ORBX_BAD_ARGUMENT);
        Q = R.P; Q.world_out = nullptr; CHECK(run(&Q, 1, res, true, &why) == ORBX_BAD_ARGUMENT);
        R.edges[4] = 6; CHECK(run(&R.P, 1, res, true, &why) == ORBX_BAD_ARGUMENT); R.edges[4] = 0;
        R.edges[3] = 0; CHECK(run(&R.P, 1, res, true, &why) == ORBX_BAD_ARGUMENT); R.edges[3] = 2;
        R.edges[5] = 2; CHECK(run(&R.P, 1, res, true, &why) == ORBX_BAD_ARGUMENT); R.edges[5] = 0;
        R.Scw[15] = 0.0; CHECK(run(&R.P, 1, res, true, &why) == ORBX_BAD_ARGUMENT); R.Scw[15] = 1.0;
        R.Scw[9] = NAN; CHECK(run(&R.P, 1, res, true, &why) == ORBX_BAD_ARGUMENT); R.Scw[9] = 0.0;
        R.ref[0] = 6; CHECK(run(&R.P, 1, res, true, &why) == ORBX_BAD_ARGUMENT); R.ref[0] = 0;
        for (double v : R.Sout) CHECK(v == 7.5);
        for (float v : R.wout) CHECK(v == 7.5f);
        CHECK(run(&R.P, 1, res, false, &why) == ORBX_OK);
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
