// orbx_essgraph.cpp -- host side of the batched Optimizer::OptimizeEssentialGraph (orbx_essgraph.h): validation of a call, the
// elimination order and the symbolic factorisation of every problem, the packing of all problems into one staging block, the
// library's host path -- the header's phases run by a plain loop over the same packed block, the problems one after the other
// -- and the scatter of the result block.  HIP-free: tools/san_essgraph.cpp builds it alone under the sanitizers.  The entry
// point (orbx_map_batches.cpp) owns the staging block and the launches.
#include <algorithm>
#include <cstring>
#include <iterator>
#include <map>
#include <set>
#include <utility>
#include "orbx_essgraph.h"

// The order is made in rounds.  In a round the vertices still in the block graph are walked by ascending (current degree,
// vertex index) and a vertex is taken when none of its neighbours has been taken in this round: an independent set, eliminated
// in the order taken.  Eliminating v joins its neighbours pairwise (the fill) and gives column v of L the rows of those
// neighbours.  Independent vertices do not see each other's fill, so the columns of a round depend on earlier rounds only.
void orbx_eg_symbolic(int nv, int ne, const int32_t *edges, const uint8_t *fixed, long long max_blocks, OrbxEgSymbolic &sym) {
    sym = OrbxEgSymbolic();
    std::vector<uint8_t> has((size_t)nv, 0);
    for (int e = 0; e < ne; ++e) { has[edges[3 * e]] = 1; has[edges[3 * e + 1]] = 1; }
    std::vector<int32_t> active;
    for (int v = 0; v < nv; ++v) if (!fixed[v] && has[v]) active.push_back(v);
    const int na = (int)active.size();
    std::vector<std::set<int32_t>> adj((size_t)nv);
    for (int e = 0; e < ne; ++e) {
        const int i = edges[3 * e], j = edges[3 * e + 1];
        if (fixed[i] || fixed[j]) continue;
        adj[i].insert(j); adj[j].insert(i);
    }
    sym.acol.assign((size_t)nv, -1);
    sym.col_vertex.clear();
    sym.round_begin.assign(1, 0);
    std::vector<std::vector<int32_t>> rows;                    // per column: the row VERTICES of its off-diagonal blocks
    std::vector<int32_t> left(active), taken, order;
    std::vector<uint8_t> blocked((size_t)nv, 0);
    long long nblocks = 0;
    while (!left.empty()) {
        order = left;
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
            return adj[a].size() != adj[b].size() ? adj[a].size() < adj[b].size() : a < b;
        });
        taken.clear();
        for (int32_t v : order) {
            if (blocked[v]) continue;
            taken.push_back(v);
            for (int32_t u : adj[v]) blocked[u] = 1;
        }
        for (int32_t v : order) blocked[v] = 0;
        for (int32_t v : taken) {
            sym.acol[v] = (int32_t)sym.col_vertex.size();
            sym.col_vertex.push_back(v);
            rows.emplace_back(adj[v].begin(), adj[v].end());
            nblocks += 1 + (long long)adj[v].size();
            if (max_blocks >= 0 && nblocks > max_blocks) { sym.over_cap = true; return; }
            for (int32_t a : adj[v]) adj[a].erase(v);
            for (auto a = adj[v].begin(); a != adj[v].end(); ++a)
                for (auto b = std::next(a); b != adj[v].end(); ++b) { adj[*a].insert(*b); adj[*b].insert(*a); }
            adj[v].clear();
        }
        std::vector<int32_t> rest;
        for (int32_t v : left) if (sym.acol[v] < 0) rest.push_back(v);
        left.swap(rest);
        sym.round_begin.push_back((int32_t)sym.col_vertex.size());
    }
    // incident edges by column, ascending edge index
    std::vector<int32_t> cnt((size_t)na + 1, 0);
    for (int e = 0; e < ne; ++e)
        for (int s = 0; s < 2; ++s) { const int c = sym.acol[edges[3 * e + s]]; if (c >= 0) ++cnt[(size_t)c + 1]; }
    for (int c = 0; c < na; ++c) cnt[(size_t)c + 1] += cnt[c];
    sym.inc_begin = cnt;
    sym.inc.assign((size_t)cnt[na], 0);
    std::vector<int32_t> pos(cnt);
    for (int e = 0; e < ne; ++e)
        for (int s = 0; s < 2; ++s) { const int c = sym.acol[edges[3 * e + s]]; if (c >= 0) sym.inc[pos[c]++] = 2 * e + s; }
    // blocks by column: the diagonal one, then the rows ascending (in elimination order)
    std::map<std::pair<int32_t, int32_t>, int32_t> index;     // (row column, column column) -> block
    sym.blk_begin.assign(1, 0);
    for (int c = 0; c < na; ++c) {
        std::vector<int32_t> r;
        for (int32_t v : rows[c]) r.push_back(sym.acol[v]);
        std::sort(r.begin(), r.end());
        index[{c, c}] = (int32_t)(sym.blk_ij.size() / 2);
        sym.blk_ij.push_back(c); sym.blk_ij.push_back(c);
        for (int32_t i : r) { index[{i, c}] = (int32_t)(sym.blk_ij.size() / 2); sym.blk_ij.push_back(i); sym.blk_ij.push_back(c); }
        sym.blk_begin.push_back((int32_t)(sym.blk_ij.size() / 2));
    }
    const int nb = (int)(sym.blk_ij.size() / 2);
    // off-diagonal blocks by row, column ascending
    std::vector<std::vector<int32_t>> by_row((size_t)na);
    for (int b = 0; b < nb; ++b) if (sym.blk_ij[2 * b] != sym.blk_ij[2 * b + 1]) by_row[sym.blk_ij[2 * b]].push_back(b);
    sym.row_begin.assign(1, 0);
    for (int c = 0; c < na; ++c) {                             // (blocks are numbered by column, so each list ascends already)
        for (int32_t b : by_row[c]) sym.row_blk.push_back(b);
        sym.row_begin.push_back((int32_t)sym.row_blk.size());
    }
    // the pairs (L(i, k), L(j, k)) of every block (i, j), k ascending: walk the two rows' lists
    sym.pair_begin.assign(1, 0);
    for (int b = 0; b < nb; ++b) {
        const int i = sym.blk_ij[2 * b], j = sym.blk_ij[2 * b + 1];
        int a = sym.row_begin[i], z = sym.row_begin[j];
        while (a < sym.row_begin[i + 1] && z < sym.row_begin[j + 1]) {
            const int ka = sym.blk_ij[2 * sym.row_blk[a] + 1], kz = sym.blk_ij[2 * sym.row_blk[z] + 1];
            if (ka >= j || kz >= j) break;
            if (ka < kz) ++a;
            else if (kz < ka) ++z;
            else { sym.pair.push_back(sym.row_blk[a]); sym.pair.push_back(sym.row_blk[z]); ++a; ++z; }
        }
        sym.pair_begin.push_back((int32_t)(sym.pair.size() / 2));
    }
    // an off-diagonal block's edges, ascending edge index, with the side of the row vertex
    std::vector<std::vector<int32_t>> ent((size_t)nb);
    for (int e = 0; e < ne; ++e) {
        const int ci = sym.acol[edges[3 * e]], cj = sym.acol[edges[3 * e + 1]];
        if (ci < 0 || cj < 0) continue;
        const int row = std::max(ci, cj), col = std::min(ci, cj);
        ent[index[{row, col}]].push_back(2 * e + (ci == row ? 0 : 1));
    }
    sym.aent_begin.assign(1, 0);
    for (int b = 0; b < nb; ++b) {
        for (int32_t v : ent[b]) sym.aent.push_back(v);
        sym.aent_begin.push_back((int32_t)sym.aent.size());
    }
}

static bool eg_finite8(const double *s) {
    for (int k = 0; k < 8; ++k) if (!orbx_finite(s[k])) return false;
    return true;
}

orbx_status orbx_eg_plan(int nproblems, const orbx_essgraph_problem *problems, const orbx_essgraph_result *results, bool cap,
                         OrbxEgPlan &plan, const char **why) {
    plan = OrbxEgPlan();
    if (nproblems < 0) { *why = "nproblems < 0"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !problems) { *why = "null problem array"; return ORBX_BAD_ARGUMENT; }
    if (nproblems > 0 && !results) { *why = "null result array"; return ORBX_BAD_ARGUMENT; }
    plan.probs.resize((size_t)nproblems);
    plan.sym.resize((size_t)nproblems);
    size_t in = orbx_pad256((size_t)nproblems * sizeof(DEgProb)), work = 0;
    size_t out = orbx_pad256((size_t)nproblems * sizeof(orbx_essgraph_result));   // the output block starts with the results
    int64_t npts = 0;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_essgraph_problem &P = problems[k];
        if (P.nvertices < 0 || P.nedges < 0 || P.npoints < 0) { *why = "a negative count"; return ORBX_BAD_ARGUMENT; }
        if (P.nvertices > ORBX_EG_MAX_VERTICES) { *why = "more than 2^20 vertices in a problem"; return ORBX_UNSUPPORTED; }
        if (P.nedges > ORBX_EG_MAX_EDGES) { *why = "more than 2^22 edges in a problem"; return ORBX_UNSUPPORTED; }
        if (P.nvertices > 0 && (!P.Scw || !P.fixed || !P.Siw_out || !P.Tiw_out)) { *why = "null Scw, fixed, Siw_out or Tiw_out"; return ORBX_BAD_ARGUMENT; }
        if ((P.non_corrected == nullptr) != (P.has_non_corrected == nullptr)) { *why = "non_corrected without has_non_corrected, or the reverse"; return ORBX_BAD_ARGUMENT; }
        if (P.nedges > 0 && !P.edges) { *why = "null edges"; return ORBX_BAD_ARGUMENT; }
        if (P.npoints > 0 && (!P.world || !P.ref || !P.world_out)) { *why = "null world, ref or world_out"; return ORBX_BAD_ARGUMENT; }
        for (int v = 0; v < P.nvertices; ++v) {
            if (!eg_finite8(P.Scw + 8 * (size_t)v)) { *why = "a non-finite Scw"; return ORBX_BAD_ARGUMENT; }
            if (!(P.Scw[8 * (size_t)v + 7] > 0)) { *why = "Scw with s <= 0"; return ORBX_BAD_ARGUMENT; }
            if (P.has_non_corrected && P.has_non_corrected[v]) {
                if (!eg_finite8(P.non_corrected + 8 * (size_t)v)) { *why = "a non-finite non_corrected"; return ORBX_BAD_ARGUMENT; }
                if (!(P.non_corrected[8 * (size_t)v + 7] > 0)) { *why = "non_corrected with s <= 0"; return ORBX_BAD_ARGUMENT; }
            }
        }
        for (int e = 0; e < P.nedges; ++e) {
            const int32_t *E = P.edges + 3 * (size_t)e;
            if (E[0] < 0 || E[0] >= P.nvertices || E[1] < 0 || E[1] >= P.nvertices) { *why = "an edge outside the vertices"; return ORBX_BAD_ARGUMENT; }
            if (E[0] == E[1]) { *why = "an edge with i == j"; return ORBX_BAD_ARGUMENT; }
            if (E[2] != 0 && E[2] != 1) { *why = "an edge kind other than 0 / 1"; return ORBX_BAD_ARGUMENT; }
        }
        for (int p = 0; p < P.npoints; ++p) {
            if (P.ref[p] < -1 || P.ref[p] >= P.nvertices) { *why = "a point's ref outside [-1, nvertices)"; return ORBX_BAD_ARGUMENT; }
            for (int a = 0; a < 3; ++a)
                if (!orbx_finite((double)P.world[3 * (size_t)p + a])) { *why = "a non-finite point"; return ORBX_BAD_ARGUMENT; }
        }
        npts += P.npoints;
        if (npts > ORBX_EG_MAX_POINTS) { *why = "more than 2^28 points in a call"; return ORBX_UNSUPPORTED; }
    }
    npts = 0;
    for (int k = 0; k < nproblems; ++k) {
        const orbx_essgraph_problem &P = problems[k];
        OrbxEgSymbolic &S = plan.sym[k];
        orbx_eg_symbolic(P.nvertices, P.nedges, P.edges, P.fixed, cap ? (long long)ORBX_EG_MAX_LBLOCKS : -1, S);
        if (S.over_cap) { *why = "more than ORBX_ESSGRAPH_MAX_LBLOCKS blocks in L (the device workspace); the host path has no cap"; return ORBX_CAPACITY; }
        DEgProb &D = plan.probs[k];
        memset(&D, 0, sizeof(D));
        D.nv = P.nvertices; D.ne = P.nedges; D.nact = (int32_t)S.col_vertex.size(); D.nblk = (int32_t)(S.blk_ij.size() / 2);
        D.npair = (int32_t)(S.pair.size() / 2); D.naent = (int32_t)S.aent.size(); D.ninc = (int32_t)S.inc.size();
        D.nrounds = (int32_t)S.round_begin.size() - 1; D.fix_scale = P.fix_scale ? 1 : 0; D.npoints = P.npoints;
        D.pt_begin = npts;
        npts += P.npoints;
        OrbxEgCtx c;
        const OrbxEgSizes s = orbx_eg_bind(D, nullptr, nullptr, nullptr, c);
        D.o_in = (int64_t)in; D.o_work = (int64_t)work; D.o_out = (int64_t)out;
        in += s.in_bytes; work += s.work_bytes; out += s.out_bytes;
    }
    plan.nproblems = nproblems;
    plan.npoints = npts;
    plan.o_pts_in = in;
    in += orbx_pad256((size_t)npts * 20);                      // world [3] float | ref | problem
    plan.o_pts_out = out;
    out += orbx_pad256((size_t)npts * 12);
    plan.in_bytes = in; plan.work_bytes = work; plan.out_bytes = out;
    return ORBX_OK;
}

template <class T> static void eg_copy(const void *dst, const std::vector<T> &v) {
    if (!v.empty()) memcpy((void *)dst, v.data(), v.size() * sizeof(T));
}

void orbx_eg_pack(const orbx_essgraph_problem *problems, const OrbxEgPlan &plan, uint8_t *dst) {
    if (plan.nproblems > 0) memcpy(dst + plan.o_prob, plan.probs.data(), (size_t)plan.nproblems * sizeof(DEgProb));
    float *world = (float *)(dst + plan.o_pts_in);
    int32_t *ref = (int32_t *)(world + 3 * (size_t)plan.npoints), *pprob = ref + plan.npoints;
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_essgraph_problem &P = problems[k];
        const DEgProb &D = plan.probs[k];
        const OrbxEgSymbolic &S = plan.sym[k];
        OrbxEgCtx c;
        orbx_eg_bind(D, dst + D.o_in, nullptr, nullptr, c);
        const size_t nv = (size_t)D.nv;
        if (nv) memcpy((void *)c.Scw, P.Scw, 64 * nv);
        double *snc = (double *)c.Snc;
        for (size_t v = 0; v < nv; ++v)
            memcpy(snc + 8 * v, (P.has_non_corrected && P.has_non_corrected[v] ? P.non_corrected : P.Scw) + 8 * v, 64);
        if (D.ne) memcpy((void *)c.edges, P.edges, 12 * (size_t)D.ne);
        eg_copy(c.acol, S.acol); eg_copy(c.col_vertex, S.col_vertex); eg_copy(c.inc_begin, S.inc_begin); eg_copy(c.inc, S.inc);
        eg_copy(c.round_begin, S.round_begin); eg_copy(c.blk_begin, S.blk_begin); eg_copy(c.blk_ij, S.blk_ij);
        eg_copy(c.pair_begin, S.pair_begin); eg_copy(c.pair, S.pair); eg_copy(c.aent_begin, S.aent_begin); eg_copy(c.aent, S.aent);
        eg_copy(c.row_begin, S.row_begin); eg_copy(c.row_blk, S.row_blk);
        if (D.npoints) {
            memcpy(world + 3 * (size_t)D.pt_begin, P.world, 12 * (size_t)D.npoints);
            memcpy(ref + D.pt_begin, P.ref, 4 * (size_t)D.npoints);
            for (int p = 0; p < D.npoints; ++p) pprob[D.pt_begin + p] = k;
        }
    }
}

namespace {
struct EgExHost {
    template <class F> void each(int n, F f) { for (int i = 0; i < n; ++i) f(i); }
    void sync() {}
    bool lead() const { return true; }
};
}  // namespace

void orbx_eg_host_run(const OrbxEgPlan &plan, const uint8_t *in, uint8_t *work, uint8_t *out) {
    orbx_essgraph_result *res = (orbx_essgraph_result *)out;
    const DEgProb *dp = (const DEgProb *)(in + plan.o_prob);
    for (int k = 0; k < plan.nproblems; ++k) {
        OrbxEgCtx c;
        orbx_eg_bind(dp[k], in + dp[k].o_in, work + dp[k].o_work, out + dp[k].o_out, c);
        EgExHost ex;
        orbx_eg_run(ex, c, &res[k]);
    }
    const float *world = (const float *)(in + plan.o_pts_in);
    const int32_t *ref = (const int32_t *)(world + 3 * (size_t)plan.npoints), *pprob = ref + plan.npoints;
    for (int64_t i = 0; i < plan.npoints; ++i) orbx_eg_correct_point(dp, in, out, world, ref, pprob, (float *)(out + plan.o_pts_out), i);
}

void orbx_eg_unpack(const orbx_essgraph_problem *problems, const OrbxEgPlan &plan, const uint8_t *out, orbx_essgraph_result *results) {
    const orbx_essgraph_result *res = (const orbx_essgraph_result *)out;
    const float *wout = (const float *)(out + plan.o_pts_out);
    for (int k = 0; k < plan.nproblems; ++k) {
        const orbx_essgraph_problem &P = problems[k];
        const DEgProb &D = plan.probs[k];
        OrbxEgCtx c;
        orbx_eg_bind(D, nullptr, nullptr, (uint8_t *)out + D.o_out, c);
        results[k] = res[k];
        if (D.nv) { memcpy(P.Siw_out, c.Siw_out, 64 * (size_t)D.nv); memcpy(P.Tiw_out, c.Tiw_out, 64 * (size_t)D.nv); }
        if (D.npoints) memcpy(P.world_out, wout + 3 * (size_t)D.pt_begin, 12 * (size_t)D.npoints);
    }
}

extern "C" double orbx_essgraph_log(double x) { return orbx_eg_logd(x); }
extern "C" void orbx_essgraph_sim3_log(const double *S8, double *out7) { orbx_eg_log(orbx_sim3opt_fetch(S8), out7); }
extern "C" void orbx_essgraph_sim3_from_tcw(const float *Tcw, double *S8) {
    double m[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) m[3 * r + c] = (double)Tcw[4 * r + c];
    OrbxSim3 S;
    orbx_pose_quat_from_R(m, S.q);
    S.q.tx = (double)Tcw[3]; S.q.ty = (double)Tcw[7]; S.q.tz = (double)Tcw[11];
    S.s = 1.0;
    orbx_sim3opt_store(S, S8);
}
