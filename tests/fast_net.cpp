// fast_net.cpp -- orbx_fast_net (csrc/orbx_fast_net.h), the corner test and score network of k_fast_rows, against the definition
// written out directly: the maximum over the 16 arcs of the minimum over the arc's 9 pixels of +-(ring - v), both polarities.
// Host only; built with -fsanitize=address,undefined by tests/test_fast_net.py.
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_fast_net.h"

static long g_cases = 0, g_fails = 0, g_corners[2] = {0, 0}, g_reruns = 0, g_rerun_corners = 0, g_ties = 0, g_tie_corners = 0;

// margin of one polarity by the definition (pol = +1: ring brighter than the centre, -1: darker)
static int margin_direct(int v, const int *x, int pol) {
    int best = -1000;
    for (int k = 0; k < 16; ++k) {
        int m = 1000;
        for (int j = 0; j < 9; ++j) m = std::min(m, pol * (x[(k + j) & 15] - v));
        best = std::max(best, m);
    }
    return best;
}

static void fail(const char *what, int v, const int *x, int th, int other) {
    if (++g_fails > 20) return;
    printf("FAIL %s: v=%d th=%d other=%d ring=", what, v, th, other);
    for (int k = 0; k < 16; ++k) printf("%d ", x[k]);
    printf("\n");
}

// one candidate: the network for both values of `other` against the definition, then the selection rule of fr_round
static void check(int v, const int *x, int th) {
    ofn_u16 xs[16];
    for (int k = 0; k < 16; ++k) xs[k] = (ofn_u16)x[k];
    const int mar[2] = {margin_direct(v, x, +1), margin_direct(v, x, -1)};   // [0] brighter, [1] darker
    const int mb = std::min(std::max(x[0], x[8]), std::max(x[4], x[12])) - v;
    const int md = v - std::max(std::min(x[0], x[8]), std::min(x[4], x[12]));
    const bool both_ref = std::min(mb, md) > th;
    bool corner[2], both[2];
    uint8_t score[2];
    for (int other = 0; other < 2; ++other) {
        ++g_cases;
        orbx_fast_net((ofn_u16)v, xs, (ofn_i16)th, other != 0, corner[other], score[other], both[other]);
        const int p = (md > mb) != (other != 0) ? 1 : 0;                    // darker iff md > mb; a tie goes to brighter
        if (corner[other] != (mar[p] > th)) fail("corner", v, x, th, other);
        else if (corner[other] && score[other] != (uint8_t)(mar[p] - 1)) fail("score", v, x, th, other);
        if (both[other] != both_ref) fail("both", v, x, th, other);
        // a lane without an entry carries the threshold 0x4000: nothing reaches it (3 cases of 16: the check costs a network)
        if ((g_cases & 15) > 2) continue;
        bool c2, b2;
        uint8_t s2;
        orbx_fast_net((ofn_u16)v, xs, (ofn_i16)0x4000, other != 0, c2, s2, b2);
        if (c2 || b2) fail("unreachable threshold", v, x, 0x4000, other);
    }
    if (mb == md) { ++g_ties; g_tie_corners += corner[0]; }
    // selection: a corner is found by the polarity with the larger compass margin, or, when both pre-tests pass, by the other one
    const bool ref_corner = std::max(mar[0], mar[1]) > th;
    bool got = corner[0];
    int got_score = score[0];
    if (!corner[0] && both[0]) {
        ++g_reruns;
        got = corner[1];
        got_score = score[1];
        g_rerun_corners += corner[1];
    }
    if (got != ref_corner) fail("selection", v, x, th, -1);
    else if (got && got_score != std::max(mar[0], mar[1]) - 1) fail("selected score", v, x, th, -1);
    if (ref_corner) ++g_corners[mar[1] > mar[0]];
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {   // xorshift64*
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545f4914f6cdd1dull) >> 32);
}

int main() {
    const int ths[6] = {0, 1, 7, 20, 254, 255};
    // ---- planted arcs: every arc start x both polarities, the arc's margin at th - 1, th, th + 1; the 7 other pixels equal to the
    // centre, at the far end of the range, or random on the far side
    long planted = 0, planted_exact[2][2] = {{0, 0}, {0, 0}};   // [polarity][margin == th + 1]
    for (int ti = 0; ti < 6; ++ti)
        for (int k = 0; k < 16; ++k)
            for (int pol = 0; pol < 2; ++pol)
                for (int dt = -1; dt <= 1; ++dt) {
                    const int th = ths[ti], t = th + dt;
                    if (t < 0 || t > 255) continue;   // th - 1 = -1 is the other polarity's business; 256 is not representable in 8 bits
                    const int vs[2] = {pol == 0 ? 0 : 255, pol == 0 ? 255 - t : t};
                    for (int vi = 0; vi < 2; ++vi)
                        for (int fill = 0; fill < 3; ++fill) {
                            const int v = vs[vi];
                            int x[16];
                            for (int j = 0; j < 16; ++j) {
                                const bool in_arc = ((j - k) & 15) < 9;
                                const int far = pol == 0 ? 0 : 255;
                                x[j] = in_arc ? (pol == 0 ? v + t : v - t) : fill == 0 ? v : fill == 1 ? far : (pol == 0 ? (int)(rnd() % (uint32_t)(v + 1)) : v + (int)(rnd() % (uint32_t)(256 - v)));
                            }
                            // every other arc holds a pixel that is not on the arc's side of the centre: the margin IS t
                            if (margin_direct(v, x, pol == 0 ? +1 : -1) != t) fail("planted margin", v, x, th, pol);
                            check(v, x, th);
                            ++planted;
                            if (dt >= 0) ++planted_exact[pol][dt];
                        }
                }
    // ---- centre and ring at 0 and 255: all 65 536 rings
    for (int bits = 0; bits < 65536; ++bits) {
        int x[16];
        for (int j = 0; j < 16; ++j) x[j] = (bits >> j) & 1 ? 255 : 0;
        const int vv[3] = {0, 255, 128};
        for (int vi = 0; vi < 3; ++vi)
            for (int ti = 0; ti < 6; ++ti) check(vv[vi], x, ths[ti]);
    }
    // ---- ties mb == md: ring pixels at v - a or v + a
    const int amps[4] = {1, 8, 21, 127};
    for (int ai = 0; ai < 4; ++ai)
        for (int bits = 0; bits < 65536; ++bits) {
            int x[16];
            for (int j = 0; j < 16; ++j) x[j] = 128 + ((bits >> j) & 1 ? amps[ai] : -amps[ai]);
            check(128, x, ai == 0 ? 0 : ai == 1 ? 7 : 20);
        }
    const long ties_planted = g_ties;
    // ---- random rings: uniform, quantised to plateaus, and close to the centre
    const int rths[7] = {0, 1, 7, 20, 100, 254, 255};
    for (long i = 0; i < 2000000; ++i) {
        int x[16];
        const int kind = (int)(i % 4);
        int v = (int)(rnd() & 255);
        if (kind == 3 && (i & 4)) v = (i & 8) ? 0 : 255;
        for (int j = 0; j < 16; ++j) {
            const int r = (int)(rnd() & 255);
            x[j] = kind == 0 ? r : kind == 1 ? r / 48 * 48 : kind == 2 ? std::min(255, std::max(0, v + r % 61 - 30)) : r / 85 * 85;
        }
        if (kind == 1) v = v / 48 * 48;
        check(v, x, kind == 2 ? rths[rnd() % 4] : rths[rnd() % 7]);
    }
    printf("planted %ld (margin th: %ld / %ld, th + 1: %ld / %ld), ties %ld (%ld planted, %ld corners), corners %ld brighter / %ld darker, "
           "re-runs %ld (%ld corners)\n", planted, planted_exact[0][0], planted_exact[1][0], planted_exact[0][1], planted_exact[1][1],
           g_ties, ties_planted, g_tie_corners, g_corners[0], g_corners[1], g_reruns, g_rerun_corners);
    // the cases must exist: a check that nothing reached proves nothing
    if (planted_exact[0][0] == 0 || planted_exact[1][0] == 0 || planted_exact[0][1] == 0 || planted_exact[1][1] == 0 || ties_planted == 0 ||
        g_tie_corners == 0 || g_corners[0] == 0 || g_corners[1] == 0 || g_rerun_corners == 0) {
        printf("FAIL vacuous\n");
        ++g_fails;
    }
    printf("%ld cases, %ld failures\n", g_cases, g_fails);
    return g_fails != 0;
}
