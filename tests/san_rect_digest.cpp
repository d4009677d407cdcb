// san_rect_digest.cpp -- the host digest of cv::remap's float maps (include/orbx_rect_digest.h: what orbx_set_rectification
// uploads and orbx_debug_rect_digest returns) under -fsanitize=address,undefined, built and run by tests/test_frontend_cpu.py.
// Host only.
//
//   * every file named on the command line holds one planted map scene of tests/frontend_scenes.py and the model's answer:
//     int64 n, float map_x[n], float map_y[n], uint32 xy[n], uint32 frac[n].  The digest runs on heap buffers of exactly n
//     entries (so AddressSanitizer sees any access past them) and must equal the model's words;
//   * a zero-length map: nothing may be read or written (the buffers have no bytes);
//   * the non-finite and out-of-range values, where a cast of lrintf's 64-bit result would be undefined or wrap: INT_MIN;
//   * every k / 64 for k in [-70000, 70000] (exact in float) against round-half-to-even in integers.
// Prints the number of failures; exit status 1 if there is one.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "../include/orbx_rect_digest.h"

static long g_fail = 0, g_checked = 0;
#define CHECK(c, ...) do { ++g_checked; if (!(c)) { if (g_fail++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// heap arrays of exactly n elements (n == 0: a zero-byte allocation nothing may touch)
template <class T> struct Heap {
    T *p; explicit Heap(size_t n) : p((T *)malloc(n * sizeof(T))) {} ~Heap() { free(p); }
    Heap(const Heap &) = delete; Heap &operator=(const Heap &) = delete;
};

static void run_file(const char *path) {
    FILE *f = fopen(path, "rb");
    CHECK(f != nullptr, "cannot open %s", path);
    if (!f) return;
    int64_t n = -1;
    CHECK(fread(&n, sizeof(n), 1, f) == 1 && n >= 0 && n < (1 << 26), "%s: header", path);
    if (n < 0) { fclose(f); return; }
    Heap<float> mx(n), my(n);
    Heap<uint32_t> exy(n), efr(n), xy(n), fr(n);
    const bool ok = fread(mx.p, 4, n, f) == (size_t)n && fread(my.p, 4, n, f) == (size_t)n && fread(exy.p, 4, n, f) == (size_t)n &&
                    fread(efr.p, 4, n, f) == (size_t)n;
    fclose(f);
    CHECK(ok, "%s: short file", path);
    if (!ok) return;
    memset(xy.p, 0xA5, n * 4); memset(fr.p, 0xA5, n * 4);
    orbx_rect_digest(mx.p, my.p, (size_t)n, xy.p, fr.p, 1);
    for (int64_t i = 0; i < n; ++i)
        CHECK(xy.p[i] == exy.p[i] && fr.p[i] == efr.p[i], "%s entry %lld (%g, %g): %08x %03x, model %08x %03x", path, (long long)i,
              (double)mx.p[i], (double)my.p[i], xy.p[i], fr.p[i], exy.p[i], efr.p[i]);
    // the interleaved form orbx_set_rectification uses: the same words, two apart
    Heap<uint32_t> il(2 * n);
    orbx_rect_digest(mx.p, my.p, (size_t)n, il.p, il.p + 1, 2);
    for (int64_t i = 0; i < n; ++i) CHECK(il.p[2 * i] == exy.p[i] && il.p[2 * i + 1] == efr.p[i], "%s interleaved entry %lld", path, (long long)i);
    printf("%s: %lld entries\n", path, (long long)n);
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) run_file(argv[a]);
    {   // zero-length map
        Heap<float> mx(0), my(0);
        Heap<uint32_t> xy(0), fr(0);
        orbx_rect_digest(mx.p, my.p, 0, xy.p, fr.p, 1);
        orbx_rect_digest(mx.p, my.p, 0, xy.p, fr.p, 2);
    }
    {   // the integer indefinite
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        const float bad[] = {nan, -nan, inf, -inf, 67108864.f, -67108864.f, 134217728.f, -134217728.f, 7e7f, -7e7f, 1e9f, -1e9f,
                             3.0e38f, -3.0e38f};
        for (float v : bad) {
            CHECK(orbx_cv_round32(v * 32.f) == INT_MIN, "cvRound(%g * 32)", (double)v);
            uint32_t xy = 0, fr = ~0u;
            orbx_rect_digest_entry(v, 3.25f, &xy, &fr);
            CHECK(xy == (0x8000u | (3u << 16)) && fr == (8u << 5), "x = %g: %08x %03x", (double)v, xy, fr);
            orbx_rect_digest_entry(3.25f, v, &xy, &fr);
            CHECK(xy == (3u | (0x8000u << 16)) && fr == 8u, "y = %g: %08x %03x", (double)v, xy, fr);
        }
        CHECK(orbx_cv_round32(2147483520.f) == 2147483520 && orbx_cv_round32(-2147483648.f) == INT_MIN, "the ends of the int range");
    }
    for (int k = -70000; k <= 70000; ++k) {   // map = k / 64: s = k / 2 rounded half to even
        int s = (k - (((k % 2) + 2) % 2)) / 2;                  // floor(k / 2)
        if (k % 2 != 0 && (s & 1)) ++s;                         // the tie goes to the even neighbour
        const int i = s >> 5, f = s & 31;
        uint32_t xy = 0, fr = 0;
        orbx_rect_digest_entry((float)k / 64.f, (float)-k / 64.f, &xy, &fr);
        int sn = (-k - (((-k % 2) + 2) % 2)) / 2;
        if (k % 2 != 0 && (sn & 1)) ++sn;
        CHECK((int)(int16_t)(xy & 0xffff) == i && (int)(fr & 31) == f, "k = %d: ix %d fx %d, expected %d %d", k, (int)(int16_t)(xy & 0xffff), (int)(fr & 31), i, f);
        CHECK((int)(int16_t)(xy >> 16) == (sn >> 5) && (int)(fr >> 5) == (sn & 31), "k = %d: y half", k);
    }
    printf("%ld checks, %ld failures\n", g_checked, g_fail);
    return g_fail ? 1 : 0;
}
