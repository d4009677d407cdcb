// orbx_newpoints.cpp -- host side of the batched per-match geometry of LocalMapping::CreateNewMapPoints (orbx_newpoints.h):
// validation of a call, the packing of all problems into one staging block (the two cameras per problem, the chunk table, and per
// match the operands gathered by index into ORBX_NEWPTS_PLANES planes), the library's host path -- the header's scalar code
// compiled by the host compiler over the same packed block, problem after problem, match after match -- and the scatter of the
// result block.  HIP-free: tests/san_newpoints.cpp builds it alone under the sanitizers.  The entry point
// (orbx_map_batches.cpp) owns the staging block and the launch.
#include <cstring>
#include "orbx_newpoints.h"

static const char *keyframe_fault(const orbx_newpoints_keyframe &K) {
    if (K.n < 0) return "a negative feature count";
    if (K.nlevels < 0) return "a negative level count";
    if (K.nlevels > 0 && (!K.scale_factors || !K.level_sigma2)) return "null scale_factors or level_sigma2";
    if (K.n > 0 && (!K.keys_un || !K.keys || !K.u_right || !K.depth)) return "null keys_un, keys, u_right or depth";
    return nullptr;
}

orbx_status orbx_newpoints_plan(int nproblems, const orbx_newpoints_problem *problems, const uint8_t *status_out,
                                const float *points_out, OrbxNewPtsPlan &plan, const char **why) {
    plan = OrbxNewPtsPlan();
    if (nproblems < 0) { *why = "nproblems < 0"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !problems) { *why = "null problem array"; return ORBX_BAD_ARGUMENT; }
    size_t total = 0, nchunks = 0;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_newpoints_problem &P = problems[k];
        if (P.nmatches < 0) { *why = "nmatches < 0"; return ORBX_BAD_ARGUMENT; }
        if (P.nmatches == 0) continue;                           // reads no array of the problem
        if (!P.matches) { *why = "null matches"; return ORBX_BAD_ARGUMENT; }
        const char *f = keyframe_fault(P.kf1);
        if (!f) f = keyframe_fault(P.kf2);
        if (f) { *why = f; return ORBX_BAD_ARGUMENT; }
        for (int m = 0; m < P.nmatches; ++m) {
            const int32_t i1 = P.matches[2 * (size_t)m], i2 = P.matches[2 * (size_t)m + 1];
            if (i1 < 0 || i1 >= P.kf1.n || i2 < 0 || i2 >= P.kf2.n) { *why = "a match index outside its keyframe"; return ORBX_BAD_ARGUMENT; }
            const int32_t o1 = P.kf1.keys_un[i1].octave, o2 = P.kf2.keys_un[i2].octave;
            if (o1 < 0 || o1 >= P.kf1.nlevels || o2 < 0 || o2 >= P.kf2.nlevels) { *why = "an octave outside the scale tables"; return ORBX_BAD_ARGUMENT; }
        }
        total += (size_t)P.nmatches;
        nchunks += ((size_t)P.nmatches + ORBX_NEWPTS_CHUNK - 1) / ORBX_NEWPTS_CHUNK;
    }
    if (total > 0 && (!status_out || !points_out)) { *why = "null status_out or points_out"; return ORBX_BAD_ARGUMENT; }
    if (total > (size_t)0x7fffffff / ORBX_NEWPTS_PLANES) { *why = "too many matches for 32-bit offsets"; return ORBX_UNSUPPORTED; }
    plan.nproblems = nproblems;
    plan.nchunks = (int)nchunks;
    plan.total = total;
    plan.o_prob = 0;
    plan.o_chunk = orbx_pad256((size_t)nproblems * sizeof(DNewPtsProb));
    plan.o_planes = plan.o_chunk + orbx_pad256(nchunks * sizeof(DNewPtsChunk));
    plan.in_bytes = plan.o_planes + orbx_pad256(total * ORBX_NEWPTS_PLANES * sizeof(float));
    plan.o_st = 0;
    plan.o_pts = orbx_pad256(total);
    plan.out_bytes = plan.o_pts + orbx_pad256(total * 3 * sizeof(float));
    return ORBX_OK;
}

static void pack_camera(const orbx_newpoints_keyframe &K, DNewPtsCam &C) {
    memcpy(C.Rcw, K.Rcw, sizeof(C.Rcw)); memcpy(C.tcw, K.tcw, sizeof(C.tcw)); memcpy(C.Ow, K.Ow, sizeof(C.Ow));
    C.fx = K.fx; C.fy = K.fy; C.cx = K.cx; C.cy = K.cy; C.invfx = K.invfx; C.invfy = K.invfy; C.mb = K.mb; C.mbf = K.mbf;
    C.pad = 0.0f;
}

void orbx_newpoints_pack(const orbx_newpoints_problem *problems, const OrbxNewPtsPlan &plan, uint8_t *dst) {
    DNewPtsProb *dp = (DNewPtsProb *)(dst + plan.o_prob);
    DNewPtsChunk *ch = (DNewPtsChunk *)(dst + plan.o_chunk);
    float *pl = (float *)(dst + plan.o_planes);
    const size_t T = plan.total;
    size_t off = 0, c = 0;
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_newpoints_problem &P = problems[k];
        DNewPtsProb &D = dp[k];
        memset(&D, 0, sizeof(D));
        D.n = P.nmatches; D.m_off = (int32_t)off;
        if (P.nmatches == 0) continue;
        pack_camera(P.kf1, D.c1); pack_camera(P.kf2, D.c2);
        D.ratio_factor = 1.5f * P.scale_factor;                  // const float ratioFactor = 1.5f * mfScaleFactor
        for (int base = 0; base < P.nmatches; base += ORBX_NEWPTS_CHUNK) { ch[c].prob = k; ch[c].base = base; ++c; }
        for (int m = 0; m < P.nmatches; ++m) {
            const size_t g = off + (size_t)m;
            const int32_t i1 = P.matches[2 * (size_t)m], i2 = P.matches[2 * (size_t)m + 1];
            const orbx_keypoint &k1 = P.kf1.keys_un[i1], &k2 = P.kf2.keys_un[i2];
            pl[NP_UX1 * T + g] = k1.x; pl[NP_UY1 * T + g] = k1.y; pl[NP_UX2 * T + g] = k2.x; pl[NP_UY2 * T + g] = k2.y;
            pl[NP_KX1 * T + g] = P.kf1.keys[2 * (size_t)i1]; pl[NP_KY1 * T + g] = P.kf1.keys[2 * (size_t)i1 + 1];
            pl[NP_KX2 * T + g] = P.kf2.keys[2 * (size_t)i2]; pl[NP_KY2 * T + g] = P.kf2.keys[2 * (size_t)i2 + 1];
            pl[NP_UR1 * T + g] = P.kf1.u_right[i1]; pl[NP_UR2 * T + g] = P.kf2.u_right[i2];
            pl[NP_D1 * T + g] = P.kf1.depth[i1]; pl[NP_D2 * T + g] = P.kf2.depth[i2];
            pl[NP_SIG1 * T + g] = P.kf1.level_sigma2[k1.octave]; pl[NP_SIG2 * T + g] = P.kf2.level_sigma2[k2.octave];
            pl[NP_SC1 * T + g] = P.kf1.scale_factors[k1.octave]; pl[NP_SC2 * T + g] = P.kf2.scale_factors[k2.octave];
        }
        off += (size_t)P.nmatches;
    }
}

void orbx_newpoints_host_run(const OrbxNewPtsPlan &plan, const uint8_t *in, uint8_t *out) {
    const DNewPtsProb *dp = (const DNewPtsProb *)(in + plan.o_prob);
    const float *pl = (const float *)(in + plan.o_planes);
    uint8_t *st = out + plan.o_st;
    float *pts = (float *)(out + plan.o_pts);
    const long long T = (long long)plan.total;
    for (int k = 0; k < plan.nproblems; ++k) {
        const DNewPtsProb &D = dp[k];
        for (int m = 0; m < D.n; ++m) {
            const long long g = (long long)D.m_off + m;
            st[g] = (uint8_t)orbx_newpoints_match(D.c1, D.c2, D.ratio_factor, orbx_newpoints_obs(pl, T, g, 0),
                                                  orbx_newpoints_obs(pl, T, g, 1), pts + 3 * g);
        }
    }
}

void orbx_newpoints_unpack(const OrbxNewPtsPlan &plan, const uint8_t *out, uint8_t *status_out, float *points_out) {
    if (plan.total == 0) return;
    memcpy(status_out, out + plan.o_st, plan.total);
    memcpy(points_out, out + plan.o_pts, plan.total * 3 * sizeof(float));
}

extern "C" float orbx_newpoints_stereo_cos(float mb, float depth) { return orbx_newpoints_stereo_cosf(mb, depth); }
