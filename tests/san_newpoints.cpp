// san_newpoints.cpp -- csrc/orbx_newpoints.cpp (validation, packing, the host path, the scatter) as a stand-alone program for
// AddressSanitizer + UndefinedBehaviorSanitizer: tests/test_newpoints_cpu.py builds it with g++ -fsanitize=address,undefined
// together with that unit and runs it.  Sizes around the chunk of 64, every stereo combination, problems without a match,
// non-finite input, every validation failure.  Prints "<n> failures".
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_newpoints.h"

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { ++failures; printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

struct Kf {
    std::vector<orbx_keypoint> un;
    std::vector<float> keys, ur, depth, sf, s2;
    orbx_newpoints_keyframe view(float ox, float mb) {
        orbx_newpoints_keyframe K = {};
        const float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int i = 0; i < 9; ++i) K.Rcw[i] = R[i];
        K.tcw[0] = -ox; K.Ow[0] = ox;
        K.fx = K.fy = 500.0f; K.cx = 320.0f; K.cy = 240.0f; K.invfx = K.invfy = 1.0f / 500.0f; K.mb = mb; K.mbf = mb * 500.0f;
        K.nlevels = (int)sf.size(); K.scale_factors = sf.data(); K.level_sigma2 = s2.data();
        K.n = (int)un.size(); K.keys_un = un.data(); K.keys = keys.data(); K.u_right = ur.data(); K.depth = depth.data();
        return K;
    }
    void add(float u, float v, int octave, float r, float d) {
        orbx_keypoint k = {u, v, 31.0f, 0.0f, 1.0f, octave, -1};
        un.push_back(k); keys.push_back(u + 0.25f); keys.push_back(v - 0.25f); ur.push_back(r); depth.push_back(d);
    }
    Kf() { float s = 1.0f; for (int l = 0; l < 8; ++l) { sf.push_back(s); s2.push_back(s * s); s *= 1.2f; } }
};

// n matches of points in front of two keyframes `baseline` apart; feature i of either keyframe is stereo by the bits of i
static void scene(int n, float baseline, Kf &a, Kf &b, std::vector<int32_t> &m, bool poison) {
    for (int i = 0; i < n; ++i) {
        const float X = -1.0f + 0.03f * (float)i, Y = 0.4f - 0.01f * (float)i, Z = 3.0f + 0.05f * (float)i;
        const float u1 = 500.0f * X / Z + 320.0f, u2 = 500.0f * (X - baseline) / Z + 320.0f, v = 500.0f * Y / Z + 240.0f;
        a.add(u1, v + (i % 9 == 8 ? 7.0f : 0.0f), i % 8, (i & 1) ? u1 - 50.0f / Z : -1.0f, (i & 1) ? Z : -1.0f);
        b.add(u2, v, (i + 1) % 8, (i & 2) ? u2 - 50.0f / Z : -1.0f, (i & 2) ? Z : -1.0f);
        m.push_back(i); m.push_back(i);
    }
    if (poison && n > 3) {
        a.un[1].x = std::numeric_limits<float>::quiet_NaN();
        a.depth[1] = std::numeric_limits<float>::infinity();
        b.un[2].y = std::numeric_limits<float>::infinity();
        b.ur[3] = 5.0f; b.depth[3] = 0.0f;                       // u_right without a depth
        a.ur[3] = std::numeric_limits<float>::quiet_NaN();
    }
}

static orbx_status run(const std::vector<orbx_newpoints_problem> &P, std::vector<uint8_t> &st, std::vector<float> &pts) {
    OrbxNewPtsPlan plan;
    const char *why = "";
    size_t total = 0;
    for (const auto &p : P) total += p.nmatches > 0 ? (size_t)p.nmatches : 0;
    st.assign(total + 1, 0xee); pts.assign(3 * total + 1, -7.0f);
    const orbx_status s = orbx_newpoints_plan((int)P.size(), P.data(), st.data(), pts.data(), plan, &why);
    if (s != ORBX_OK) return s;
    EXPECT(plan.total == total);
    std::vector<uint8_t> in(plan.in_bytes), out(plan.out_bytes);
    orbx_newpoints_pack(P.data(), plan, in.data());
    const DNewPtsChunk *ch = (const DNewPtsChunk *)(in.data() + plan.o_chunk);
    size_t covered = 0;
    for (int c = 0; c < plan.nchunks; ++c) {
        EXPECT(ch[c].prob >= 0 && ch[c].prob < (int)P.size() && ch[c].base % ORBX_NEWPTS_CHUNK == 0 && ch[c].base < P[ch[c].prob].nmatches);
        const int left = P[ch[c].prob].nmatches - ch[c].base;
        covered += (size_t)(left < ORBX_NEWPTS_CHUNK ? left : ORBX_NEWPTS_CHUNK);
    }
    EXPECT(covered == total);
    orbx_newpoints_host_run(plan, in.data(), out.data());
    orbx_newpoints_unpack(plan, out.data(), st.data(), pts.data());
    EXPECT(st[total] == 0xee && pts[3 * total] == -7.0f);
    for (size_t g = 0; g < total; ++g) {
        EXPECT(st[g] >= ORBX_NEWPOINT_TRIANGULATED && st[g] <= ORBX_NEWPOINT_NO_DEPTH);
        if (st[g] > ORBX_NEWPOINT_STEREO2) EXPECT(pts[3 * g] == 0.0f && pts[3 * g + 1] == 0.0f && pts[3 * g + 2] == 0.0f);
    }
    return s;
}

int main() {
    const int sizes[] = {1, 63, 64, 65, 129};
    std::vector<uint8_t> st;
    std::vector<float> pts;
    for (int poison = 0; poison < 2; ++poison)
        for (float baseline : {0.8f, 0.005f}) {
            std::vector<Kf> a(5), b(5);
            std::vector<std::vector<int32_t>> m(5);
            std::vector<orbx_newpoints_problem> P;
            for (int k = 0; k < 5; ++k) {
                scene(sizes[k], baseline, a[k], b[k], m[k], poison != 0);
                orbx_newpoints_problem p = {};
                p.kf1 = a[k].view(0.0f, 0.1f); p.kf2 = b[k].view(baseline, 0.3f); p.scale_factor = 1.2f;
                p.nmatches = sizes[k]; p.matches = m[k].data();
                P.push_back(p);
                if (k == 2) { orbx_newpoints_problem e = {}; P.push_back(e); }   // a problem without a match and without arrays
            }
            EXPECT(run(P, st, pts) == ORBX_OK);
            int accepted = 0;
            for (size_t g = 0; g + 1 < st.size(); ++g) accepted += st[g] <= ORBX_NEWPOINT_STEREO2;
            EXPECT(accepted > 100);
            // validation: each failure on the last problem
            orbx_newpoints_problem keep = P.back();
            OrbxNewPtsPlan plan;
            const char *why = "";
            auto bad = [&]() { return orbx_newpoints_plan((int)P.size(), P.data(), st.data(), pts.data(), plan, &why) == ORBX_BAD_ARGUMENT; };
            P.back().nmatches = -1; EXPECT(bad()); P.back() = keep;
            P.back().matches = nullptr; EXPECT(bad()); P.back() = keep;
            P.back().kf1.n = -1; EXPECT(bad()); P.back() = keep;
            P.back().kf2.nlevels = -1; EXPECT(bad()); P.back() = keep;
            P.back().kf2.depth = nullptr; EXPECT(bad()); P.back() = keep;
            P.back().kf1.level_sigma2 = nullptr; EXPECT(bad()); P.back() = keep;
            P.back().kf2.nlevels = 3; EXPECT(bad()); P.back() = keep;              // octaves run to 7
            m[4][11] = 129; EXPECT(bad()); m[4][11] = -1; EXPECT(bad()); m[4][11] = 5;
            EXPECT(orbx_newpoints_plan(-1, P.data(), st.data(), pts.data(), plan, &why) == ORBX_BAD_ARGUMENT);
            EXPECT(orbx_newpoints_plan(2, nullptr, st.data(), pts.data(), plan, &why) == ORBX_BAD_ARGUMENT);
            EXPECT(orbx_newpoints_plan((int)P.size(), P.data(), nullptr, pts.data(), plan, &why) == ORBX_BAD_ARGUMENT);
            EXPECT(orbx_newpoints_plan(0, nullptr, nullptr, nullptr, plan, &why) == ORBX_OK && plan.total == 0 && plan.nchunks == 0);
        }
    EXPECT(std::fabs(orbx_newpoints_stereo_cos(0.1f, 4.0f) - std::cos(2.0f * std::atan2(0.05f, 4.0f))) < 2e-7f);
    printf("%d failures\n", failures);
    return failures != 0;
}
