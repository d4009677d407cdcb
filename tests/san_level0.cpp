// san_level0.cpp -- CPU proof of the in-place level-0 loads (csrc/orbx_inplace.h), built with -fsanitize=address,undefined
// together with csrc/orbx_geometry.cpp by tests/test_level0_bounds.py.  Host only.
//
// For each geometry the program replays, lane by lane, the loads the three in-place consumers issue, through the SAME
// helpers the kernels use, on a heap buffer of exactly (H - 1) * stride + W bytes (so AddressSanitizer sees any over-read too):
//   * k_fast_rows_ip:          every level-0 group x staged row x lane (register window and the tall-cell loop);
//   * k_pyr_resize_rows_l1:       every column strip x lane x source row a vertical tap names;
//   * k_describe<., true>:        every level-0 keypoint position x lane.
// Checked: (1) the invariant -- every load lies inside [0, (H - 1) * stride + W) of its frame, and inside its own source row;
// (2) coverage -- what the consumer ends up with (LDS tile, selected tap bytes, LDS patch) equals the padded reflect-101
// level 0 that k_pyr_l0 would have written, at every position the consumer reads.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_internal.h"
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_inplace.h"

static long g_fail = 0, g_loads = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Img {
    int W, H, stride; size_t n; uint8_t *p;
    Img(int w, int h, int s) : W(w), H(h), stride(s), n((size_t)(h - 1) * s + w), p((uint8_t *)malloc(n)) {
        for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)((i * 2654435761u) >> 13);
    }
    ~Img() { free(p); }
    // one load of `nb` bytes at byte offset `off` that the kernel attributes to source row `row`
    void load(uint32_t off, int nb, int row, uint8_t *dst) const {
        ++g_loads;
        const bool ok = (size_t)off + nb <= n && row >= 0 && row < H && off >= (uint32_t)row * stride && off + nb <= (uint32_t)row * stride + W;
        CHECK(ok, "load off=%u nb=%d row=%d (W=%d H=%d stride=%d)", off, nb, row, W, H, stride);
        if (ok) memcpy(dst, p + off, nb); else memset(dst, 0, nb);
    }
    uint8_t raw(int y, int x) const { return p[(size_t)y * stride + x]; }
    // padded level 0, also beyond its own edges (k_describe's reflect of the padded image)
    uint8_t pad(int Y, int X) const { return raw(orbx_ip_map(Y, H), orbx_ip_map(X, W)); }
};
static uint32_t rd32(const uint8_t *b) { uint32_t v; memcpy(&v, b, 4); return v; }
static uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (s & 3))); }
static void shr96(uint32_t v[3], int s) {   // orbx_shr96
    uint32_t a = v[0], b = v[1], c = v[2];
    if (s >= 8) { a = c; b = 0; c = 0; } else if (s >= 4) { a = b; b = c; c = 0; }
    if (s >= 12) a = 0;
    v[0] = alignbyte(b, a, s & 3); v[1] = alignbyte(c, b, s & 3); v[2] = alignbyte(0, c, s & 3);
}

static const int TP = 76;   // FR_TP
static void walk_fast(const OrbxGeom &g, const Img &im) {
    std::vector<uint8_t> tile;
    for (const OrbxFastGroup &grp : g.fast_groups) {
        const OrbxCell &c0 = g.cells[grp.cell0], &c1 = g.cells[grp.cell0 + grp.ncell - 1];
        if (c0.level != 0) continue;
        const int tw = c1.x0 + c1.cw - c0.x0, rows = c0.ch;
        tile.assign((size_t)(rows + 1) * TP, 0xCD);
        int dsh;
        const int xb = orbx_ip_fast_xb(c0.x0, &dsh);
        const bool clamped = xb + 84 > im.W;
        for (int lane = 0; lane < 64; ++lane) {
            const int rq = (lane * 37) >> 8, dq = lane - 7 * rq;
            int shr;
            const int col = orbx_ip_fast_piece_col(xb, dq, im.W, &shr);
            auto stage = [&](int r, bool store) {
                const int prow = std::min(c0.y0 + r, c0.y0 + c0.ch - 1);
                const int rr = orbx_ip_fast_row(prow, im.H);
                uint8_t b[12]; uint32_t v[3];
                im.load(orbx_ip_row_off(rr, im.stride, col), 12, rr, b);
                for (int i = 0; i < 3; ++i) v[i] = rd32(b + 4 * i);
                if (clamped) shr96(v, shr);
                if (!store) return;
                uint8_t *d = &tile[(size_t)r * TP + 4 * (3 * dq + dsh)];
                if (dq < 6) memcpy(d, v, 12); else if (dsh == 0) memcpy(d, v, 4);
            };
            for (int k = 0; k < 5; ++k) stage(std::min(rq, 8) + 9 * k, rq < 9 && 9 * k + rq < rows);   // every lane loads, clamped rows included
            if (rows > 45 && rq < 9) for (int r = 45 + rq; r < rows; r += 9) stage(r, true);
        }
        const int rs = c0.x0 - ORBX_EDGE, nl = rs < 0 ? -rs : 0, nr = std::max(rs + tw - im.W, 0);
        const int p0 = 4 * dsh - xb, pW = p0 + im.W;
        for (int r = 0; r < rows; ++r) {
            uint8_t *row = &tile[(size_t)r * TP];
            for (int i = 1; i <= nl; ++i) { CHECK(p0 - i >= 0 && p0 + i < TP, "left mirror"); row[p0 - i] = row[p0 + i]; }
            for (int i = 0; i < nr; ++i) { CHECK(pW - 2 - i >= 0 && pW + i < TP, "right mirror"); row[pW + i] = row[pW - 2 - i]; }
        }
        const int off = orbx_ip_fast_tile_off(c0.x0);
        CHECK(off >= 0 && off + tw <= TP, "tile extent off=%d tw=%d", off, tw);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < tw; ++c)
                CHECK(tile[(size_t)r * TP + off + c] == im.pad(c0.y0 + r, c0.x0 + c), "FAST tile x0=%d y0=%d r=%d c=%d", c0.x0, c0.y0, r, c);
    }
}

static void walk_resize(const OrbxGeom &g, const Img &im) {
    CHECK(g.l1_inplace, "level-1 raw tap table rejected");
    if (!g.l1_inplace) return;
    const OrbxLevelGeom &L = g.lv[1];
    const OrbxTap *tx1 = &g.taps[g.l1_tap_begin], *ty1 = tx1 + L.pw;
    const OrbxTap *tx0 = &g.taps[L.tapx_begin], *ty0 = &g.taps[L.tapy_begin];
    const int nbx = (L.pw + 255) / 256;
    for (int bx = 0; bx < nbx; ++bx) {
        const bool tail = bx >= g.l1_tail_bx;
        for (int lane = 0; lane < 64; ++lane) {
            const int X = (bx * 64 + lane) * 4;
            int lo = 0x7fff;
            for (int i = 0; i < 4; ++i) { const OrbxTap &t = tx1[std::min(X + i, L.pw - 1)]; lo = std::min<int>(lo, std::min(t.s0, t.s1)); }
            const int org = tail ? orbx_ip_rr_tail_col(lo, im.W) : lo;
            const int lsrc = tail ? orbx_ip_rr_tail_col(lo, im.W) : orbx_ip_rr_body_col(lo);
            CHECK(tail || !orbx_ip_rr_window_leaves_row(lo, im.W), "body strip %d lane %d leaves the row", bx, lane);
            for (int Y = 0; Y < L.ph; ++Y)
                for (int half = 0; half < 2; ++half) {
                    const int row = half ? ty1[Y].s1 : ty1[Y].s0, prow = half ? ty0[Y].s1 : ty0[Y].s0;
                    uint8_t b[12] = {0}, reg[8];
                    const uint32_t off = orbx_ip_row_off(row, im.stride, lsrc);
                    if (tail) { im.load(off, 8, row, b); memcpy(reg, b, 8); }
                    else {
                        CHECK((off & 3) == 0, "unaligned body window");
                        im.load(off, 12, row, b);
                        const uint32_t l = alignbyte(rd32(b + 4), rd32(b), lo & 3), h = alignbyte(rd32(b + 8), rd32(b + 4), lo & 3);
                        memcpy(reg, &l, 4); memcpy(reg + 4, &h, 4);
                    }
                    for (int i = 0; i < 4 && X + i < L.pw; ++i) {
                        const OrbxTap &t = tx1[X + i], &tp = tx0[X + i];
                        const int d0 = t.s0 - org, d1 = t.s1 - org;
                        CHECK(d0 >= 0 && d0 < 8 && d1 >= 0 && d1 < 8, "selector out of the 8 bytes");
                        if (d0 < 0 || d0 > 7 || d1 < 0 || d1 > 7) continue;
                        CHECK(t.a0 == tp.a0 && t.a1 == tp.a1, "weights");
                        CHECK(reg[d0] == im.pad(prow, tp.s0), "resize tap 0 X=%d Y=%d", X + i, Y);
                        CHECK(tp.a1 == 0 || reg[d1] == im.pad(prow, tp.s1), "resize tap 1 X=%d Y=%d", X + i, Y);
                    }
                }
        }
    }
}

static const int DW = 43, DPP = 44;
static void walk_describe(const OrbxGeom &g, const Img &im, int interior_step) {
    const OrbxLevelGeom &L = g.lv[0];
    alignas(4) uint8_t patch[DW * DPP];
    long n_edge = 0, n_all = 0;
    // level-0 keypoints: padded x in [16, pw - 16), y in [16, ph - 16) (the quadtree region)
    for (int y = 16; y < L.ph - 16; ++y)
        for (int x = 16; x < L.pw - 16; ++x) {
            ++n_all;
            const int px0 = x - 21 - ORBX_EDGE, py0 = y - 21 - ORBX_EDGE;   // raw
            const bool interior = orbx_ip_desc_interior(px0, py0, im.W, im.H);
            const bool compare = !interior || ((x * 131 + y * 17) % interior_step) == 0;
            if (compare) memset(patch, 0xCD, sizeof(patch));
            uint32_t tv[64][3][3];
            const int ws = orbx_ip_desc_ws(px0, im.W), xa = px0 & ~3;
            for (int lane = 0; lane < 64; ++lane) {
                const int dq = lane & 3, rq = lane >> 2;
                for (int k = 0; k < 3; ++k) {
                    const int r = std::min(16 * k + rq, DW - 1);
                    uint8_t b[12];
                    if (interior) im.load(orbx_ip_row_off(py0 + r, im.stride, xa + 12 * dq), 12, py0 + r, b);
                    else { const int rr = orbx_ip_map(py0 + ORBX_EDGE + r, im.H); im.load(orbx_ip_row_off(rr, im.stride, ws + 12 * dq), 12, rr, b); }
                    for (int i = 0; i < 3; ++i) tv[lane][k][i] = rd32(b + 4 * i);
                }
            }
            if (!compare) continue;
            uint32_t *pd = (uint32_t *)patch;
            const int e = interior ? px0 - xa : px0 - ws, dd = e >> 2;
            const uint32_t shift = (uint32_t)(e & 3);
            for (int lane = 0; lane < 64; ++lane) {
                const int dq = lane & 3, rq = lane >> 2;
                for (int k = 0; k < 3; ++k) {
                    const int r = 16 * k + rq;
                    if (r >= DW) continue;
                    const uint32_t *t = tv[lane][k], nxt = lane < 63 ? tv[lane + 1][k][0] : 0u;
                    uint32_t *d = pd + r * (DPP / 4);
                    const uint32_t f0 = alignbyte(t[1], t[0], shift), f1 = alignbyte(t[2], t[1], shift), f2 = alignbyte(nxt, t[2], shift);
                    if (interior) { d[3 * dq] = f0; d[3 * dq + 1] = f1; if (dq < 3) d[3 * dq + 2] = f2; continue; }
                    const int D = 3 * dq - dd;
                    if (D >= 0 && D < DPP / 4) d[D] = f0;
                    if (D + 1 >= 0 && D + 1 < DPP / 4) d[D + 1] = f1;
                    if (D + 2 >= 0 && D + 2 < DPP / 4) d[D + 2] = f2;
                    if (dq == 0 && D - 1 >= 0 && D - 1 < DPP / 4) d[D - 1] = alignbyte(t[0], 0u, shift);
                }
            }
            if (!interior) {
                ++n_edge;
                const int c_end_l = px0 < 0 ? std::min(-px0, DW) : 0, c_beg_r = std::max(im.W - px0, 0);
                for (int lane = 0; lane < DW; ++lane) {
                    uint8_t *pb = patch + lane * DPP;
                    const int rr = orbx_ip_map(py0 + ORBX_EDGE + lane, im.H);
                    for (int c = 0; c < DW; ++c) {
                        if (c >= c_end_l && c < c_beg_r) continue;
                        const int j = orbx_ip_map(px0 + ORBX_EDGE + c, im.W), sp = j - px0;
                        uint8_t v;
                        if (sp >= 0 && sp < DPP) v = pb[sp]; else im.load(orbx_ip_row_off(rr, im.stride, j), 1, rr, &v);
                        pb[c] = v;
                    }
                }
            }
            for (int r = 0; r < DW; ++r)
                for (int c = 0; c < DW; ++c)
                    CHECK(patch[r * DPP + c] == im.pad(y - 21 + r, x - 21 + c), "patch x=%d y=%d r=%d c=%d interior=%d", x, y, r, c, (int)interior);
        }
    printf("  describe: %ld positions, %ld on the edge path (%.1f %%)\n", n_all, n_edge, 100.0 * n_edge / std::max(n_all, 1L));
}

int main() {
    const int geo[][3] = {{640, 480, 640}, {752, 480, 752}, {1241, 376, 1244}, {1920, 1080, 1920}, {639, 479, 640}, {97, 75, 100},
                          {ORBX_IP_MIN_W, ORBX_IP_MIN_H, ORBX_IP_MIN_W}, {67, 64, 68}, {200, 73, 200}};
    for (const auto &q : geo) {
        const int W = q[0], H = q[1], stride = q[2];
        orbx_params p;
        memset(&p, 0, sizeof(p));
        p.nfeatures = 1000; p.scale_factor = 1.2f; p.nlevels = 8; p.ini_th_fast = 20; p.min_th_fast = 7; p.max_batch = 1;
        OrbxTables t;
        OrbxGeom g;
        const char *why = "";
        orbx_build_tables(p, t);
        const orbx_status st = orbx_build_geometry(p, t, W, H, g, &why);
        printf("%dx%d stride %d: status %d\n", W, H, stride, (int)st);
        CHECK(st == ORBX_OK, "%s", why);
        if (st != ORBX_OK) continue;
        Img im(W, H, stride);
        walk_fast(g, im);
        walk_resize(g, im);
        walk_describe(g, im, W * H > 1000000 ? 97 : 13);
    }
    printf("%ld loads, %ld failures\n", g_loads, g_fail);
    return g_fail ? 1 : 0;
}
