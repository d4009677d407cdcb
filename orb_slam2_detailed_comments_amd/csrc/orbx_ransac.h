// orbx_ransac.h -- the frame the batched RANSACs share (Sim3Solver: orbx_sim3.h, PnPsolver: orbx_pnp.h, Initializer: orbx_init.h):
// the staging layout and the walk over the problems that fills it, the kernels' argument record, and the small helpers around
// set indices, mask words and stored NaNs.  Header-only and HIP-free; the numerics are each solver's own.
//
// Uploaded block (one copy): Prob[nlaunch] | hyp_prob | sets | groups | pts.  Downloaded block: hyp | masks | tally.  A problem
// that "launches" has hypotheses to compute; `groups` are the workgroups of the solver's second kernel: (problem, first
// hypothesis within the problem) pairs.  `tally` is one 4-byte value per hypothesis: the inlier count, or the Initializer's score.
#pragma once
#include <limits.h>
#include <stddef.h>
#include "orbx_lm.h"   // ORBX_HD, ORBX_UNROLL, include/orbx.h

// A NaN's sign and payload differ between processors (x86 makes 0xffc00000, gfx950 0x7fc00000), so every stored value that is
// a NaN is stored as the canonical quiet NaN: "bit for bit" then holds outside the contract too.
ORBX_HD static inline float orbx_canonf(float x) {
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    if ((b & 0x7fffffffu) > 0x7f800000u) b = 0x7fc00000u;
    __builtin_memcpy(&x, &b, 4);
    return x;
}
ORBX_HD static inline double orbx_canond(double x) {
    uint64_t b;
    __builtin_memcpy(&b, &x, 8);
    if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;
    __builtin_memcpy(&x, &b, 8);
    return x;
}
static inline size_t orbx_pad256(size_t b) { return (b + 255) & ~(size_t)255; }
// The reference converts a double to int as it is; outside int's range that conversion is undefined, so the library fixes it:
// NaN and anything at or beyond 2^31 give the largest int, anything below -2^31 the lowest.
static inline int orbx_to_int_clamped(double v) { return !(v < 2147483648.0) ? INT_MAX : v < -2147483648.0 ? INT_MIN : (int)v; }
// one drawn set of K indices: all inside [0, n) and, where the solver asks for it, no index twice
template <int K> static inline bool orbx_set_ok(const int32_t *s, int32_t n, bool distinct) {
    for (int c = 0; c < K; ++c) {
        if (s[c] < 0 || s[c] >= n) return false;
        for (int e = 0; distinct && e < c; ++e)
            if (s[e] == s[c]) return false;
    }
    return true;
}
static inline void orbx_unpack_mask(const uint64_t *words, int n, uint8_t *out) {
    for (int p = 0; p < n; ++p) out[p] = (uint8_t)((words[p >> 6] >> (p & 63)) & 1u);
}
// solver / result k of a batch, or null with *why set
template <class Batch> static inline auto *orbx_batch_state(Batch *b, int k, const char **why) {
    decltype(&b->st[0]) none = nullptr;
    if (!b) { *why = "no batch"; return none; }
    if (k < 0 || (size_t)k >= b->st.size()) { *why = "problem outside the batch"; return none; }
    return &b->st[k];
}

struct OrbxRansacPlan {
    int nproblems = 0, nlaunch = 0, total_hyps = 0, ngroups = 0;
    size_t total_sets = 0, total_pts = 0, total_words = 0;     // set ints, plane floats, mask words
    size_t o_prob = 0, o_hyp_prob = 0, o_sets = 0, o_groups = 0, o_pts = 0, in_bytes = 0;
    size_t o_hyp = 0, o_masks = 0, o_tally = 0, out_bytes = 0;
};
// the two offset ladders, from the plan's six totals and the sizes of the solver's problem and hypothesis records
static inline void orbx_ransac_layout(OrbxRansacPlan &p, size_t prob_size, size_t hyp_size) {
    p.o_prob = 0;
    p.o_hyp_prob = orbx_pad256((size_t)p.nlaunch * prob_size);
    p.o_sets = p.o_hyp_prob + orbx_pad256((size_t)p.total_hyps * sizeof(int32_t));
    p.o_groups = p.o_sets + orbx_pad256(p.total_sets * sizeof(int32_t));
    p.o_pts = p.o_groups + orbx_pad256((size_t)p.ngroups * 2 * sizeof(int32_t));
    p.in_bytes = p.o_pts + orbx_pad256(p.total_pts * sizeof(float));
    p.o_hyp = 0;
    p.o_masks = orbx_pad256((size_t)p.total_hyps * hyp_size);
    p.o_tally = p.o_masks + orbx_pad256(p.total_words * sizeof(uint64_t));
    p.out_bytes = p.o_tally + orbx_pad256((size_t)p.total_hyps * 4);
}

// The walk over the problems that launch, in order.  plan() counts with it and pack() fills with it, so where a problem's
// hypotheses, sets, planes and mask words start is decided in one place.  max_hyps / max_sets: the solver's 32-bit limits.
struct OrbxRansacWalk {
    struct At { bool ok; int32_t j, nwords, hyp_off, set_off, pts_off, word_off; };   // ok: every total is inside its limit
    size_t max_hyps, max_sets;
    int32_t *hyp_prob, *groups;                                // pack: the two index arrays, filled by add(); plan: null
    int j = 0, g = 0;
    size_t hyp_off = 0, set_off = 0, pts_off = 0, word_off = 0;
    OrbxRansacWalk(size_t max_hyps_, size_t max_sets_, int32_t *hyp_prob_ = nullptr, int32_t *groups_ = nullptr)
        : max_hyps(max_hyps_), max_sets(max_sets_), hyp_prob(hyp_prob_), groups(groups_) {}
    // the next problem that launches: n points in `planes` planes, `hyps` hypotheses drawn from set_ints indices, and one
    // workgroup of the second kernel per hyps_per_group hypotheses.  Returns where the problem's parts start.
    At add(int32_t n, size_t hyps, size_t set_ints, int planes, int hyps_per_group) {
        At at = {false, j, (n + 63) / 64, (int32_t)hyp_off, (int32_t)set_off, (int32_t)pts_off, (int32_t)word_off};
        const size_t h0 = hyp_off;
        hyp_off += hyps; set_off += set_ints; pts_off += (size_t)n * planes; word_off += hyps * (size_t)at.nwords;
        if (hyp_off > max_hyps || set_off > max_sets || pts_off > (size_t)0x3fffffff || word_off > (size_t)0x3fffffff) return at;
        for (size_t i = 0; hyp_prob && i < hyps; ++i) hyp_prob[h0 + i] = j;
        for (size_t i = 0; i < hyps; i += hyps_per_group, ++g)
            if (groups) { groups[2 * g] = j; groups[2 * g + 1] = (int32_t)i; }
        ++j;
        at.ok = true;
        return at;
    }
    OrbxRansacPlan plan(int nproblems, size_t prob_size, size_t hyp_size) const {
        OrbxRansacPlan p;
        p.nproblems = nproblems; p.nlaunch = j; p.total_hyps = (int)hyp_off; p.ngroups = g;
        p.total_sets = set_off; p.total_pts = pts_off; p.total_words = word_off;
        orbx_ransac_layout(p, prob_size, hyp_size);
        return p;
    }
};

// What the kernels of a solver get, by value; the members keep the order the three solvers' records had (hyp, tally, masks).
template <class Prob, class Hyp, class Tally> struct DRansacArgs {
    static_assert(sizeof(Tally) == 4, "the plan lays out one 4-byte tally per hypothesis");
    const Prob *prob;
    const int32_t *hyp_prob;        // [total_hyps] the problem of a hypothesis
    const int32_t *sets;
    const int32_t *groups;          // [ngroups][2]
    const float *pts;
    int total_hyps, ngroups;
    Hyp *hyp;
    Tally *tally;
    unsigned long long *masks;
};
template <class Args> static inline Args orbx_ransac_args(const OrbxRansacPlan &plan, uint8_t *in, uint8_t *out) {
    Args a;
    a.prob = (decltype(a.prob))(in + plan.o_prob);
    a.hyp_prob = (const int32_t *)(in + plan.o_hyp_prob);
    a.sets = (const int32_t *)(in + plan.o_sets);
    a.groups = (const int32_t *)(in + plan.o_groups);
    a.pts = (const float *)(in + plan.o_pts);
    a.total_hyps = plan.total_hyps; a.ngroups = plan.ngroups;
    a.hyp = (decltype(a.hyp))(out + plan.o_hyp);
    a.masks = (unsigned long long *)(out + plan.o_masks);
    a.tally = (decltype(a.tally))(out + plan.o_tally);
    return a;
}
