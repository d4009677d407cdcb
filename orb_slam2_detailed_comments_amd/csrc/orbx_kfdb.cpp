// orbx_kfdb.cpp -- the keyframe database behind the C ABI: ORB_SLAM2::KeyFrameDatabase (reference src/KeyFrameDatabase.cc)
// and DBoW2's scoring functions (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp).
//   add / erase / clear                     :56-100
//   DetectLoopCandidates                    :114-263   steps 1-3 = orbx_kfdb_query_loop,  steps 4-5 = orbx_kfdb_select_groups
//   DetectRelocalizationCandidates          :274-411   steps 1-3 = orbx_kfdb_query_reloc, steps 4-5 = orbx_kfdb_select_groups
// GPU: the common-word count and the smallest common word of every (query, entry) pair, the maximum over the listed
// entries, and the scores of the entries above the word threshold (k_kfdb_common / k_kfdb_score).  The order of
// lKFsSharingWords is first-encounter order = ascending (smallest common word, position in that word's list), and with unique
// entries and an order-preserving erase the position order is the order of the add calls: every entry's key is computed
// independently and no inverted file is needed on the device.
// Host: the order-dependent part -- sorting the sharers by that key, folding the per-entry marks / counters / scores the
// reference keeps in the KeyFrames (they persist across queries), and the covisibility groups.
// Host path (host-only handles, ORBX_KFDB=host, queries that meet an entry already marked with their id): the inverted-file
// walk exactly as the reference runs it.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include "orbx_handle.h"

namespace {
// ---- DBoW2 scoring (ScoringObject.cpp:23-315).  The lower_bound skips of the reference visit the same common words as this
// plain merge, in the same ascending order.  fma_mode: `score += vi * wi` is one fused multiply-add in a GCC -O3 -march=native
// build; the other expressions have no product feeding an addition directly.
template <class F> void walk_common(const uint32_t *aw, int na, const uint32_t *bw, int nb, F &&f) {
    int i = 0, j = 0;
    while (i < na && j < nb) {
        if (aw[i] == bw[j]) { f(i, j); ++i; ++j; }
        else if (aw[i] < bw[j]) ++i;
        else ++j;
    }
}
double bow_score(int scoring, bool fma_mode, const uint32_t *aw, const double *av, int na, const uint32_t *bw, const double *bv,
                 int nb) {
    double score = 0;
    switch (scoring) {
    case 0:   // L1Scoring (:23-68)
        walk_common(aw, na, bw, nb, [&](int i, int j) { const double vi = av[i], wi = bv[j]; score += fabs(vi - wi) - fabs(vi) - fabs(wi); });
        return -score / 2.0;
    case 1:   // L2Scoring (:73-117)
    case 5:   // DotProductScoring (:275-315)
        if (fma_mode) walk_common(aw, na, bw, nb, [&](int i, int j) { score = __builtin_fma(av[i], bv[j], score); });
        else walk_common(aw, na, bw, nb, [&](int i, int j) { score += av[i] * bv[j]; });
        if (scoring == 5) return score;
        return score >= 1 ? 1.0 : 1.0 - sqrt(1.0 - score);
    case 2:   // ChiSquareScoring (:122-166)
        walk_common(aw, na, bw, nb, [&](int i, int j) { const double vi = av[i], wi = bv[j]; if (vi + wi != 0.0) score += vi * wi / (vi + wi); });
        return 2. * score;
    case 3: { // KLScoring (:171-222): words of v1 that v2 lacks count too
        const double LOG_EPS = log(2.220446049250313e-16);   // log(DBL_EPSILON)
        int i = 0, j = 0;
        while (i < na && j < nb) {
            const double vi = av[i], wi = bv[j];
            if (aw[i] == bw[j]) {
                if (vi != 0 && wi != 0) { const double l = log(vi / wi); score = fma_mode ? __builtin_fma(vi, l, score) : score + vi * l; }
                ++i; ++j;
            } else if (aw[i] < bw[j]) {
                const double l = log(vi) - LOG_EPS;
                score = fma_mode ? __builtin_fma(vi, l, score) : score + vi * l;
                ++i;
            } else {
                ++j;   // v2.lower_bound(v1_it->first) ends at the same element as stepping does
            }
        }
        for (; i < na; ++i)
            if (av[i] != 0) { const double l = log(av[i]) - LOG_EPS; score = fma_mode ? __builtin_fma(av[i], l, score) : score + av[i] * l; }
        return score;
    }
    default:  // BhattacharyyaScoring (:227-270)
        walk_common(aw, na, bw, nb, [&](int i, int j) { score += sqrt(av[i] * bv[j]); });
        return score;
    }
}
bool bow_ok(const uint32_t *w, const double *v, int n) {
    if (n < 0 || (n > 0 && (!w || !v))) return false;
    for (int i = 1; i < n; ++i)
        if (w[i] <= w[i - 1]) return false;   // std::map order
    return true;
}

template <class T> struct DBuf {
    T *p = nullptr;
    size_t cap = 0;
    hipError_t need(size_t n) {   // contents are not kept
        if (n <= cap) return hipSuccess;
        if (p) hipFree(p);
        p = nullptr; cap = 0;
        const size_t c = n + n / 2 + 64;
        hipError_t e = hipMalloc((void **)&p, c * sizeof(T));
        if (e == hipSuccess) cap = c;
        return e;
    }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
};

// what the reference keeps in the KeyFrame: mnRelocQuery / mnRelocWords / mRelocScore [0], mnLoopQuery / mnLoopWords /
// mLoopScore [1] (KeyFrame.cc:53-56 initialises marks and counts to 0 and leaves the scores uninitialised: valid = 0)
struct KfState {
    int64_t mark[2] = {0, 0};
    int32_t words[2] = {0, 0};
    float score[2] = {0.0f, 0.0f};
    uint8_t valid[2] = {0, 0};
};
struct KfEntry {
    int64_t id = 0;
    uint64_t seq = 0;           // order of the add calls = position order inside every inverted-file list
    bool live = false;
    std::vector<uint32_t> w;
    std::vector<double> v;
};
struct KfDelta { int slot; int64_t mark; int32_t words; float score; uint8_t valid; };
struct KfMatch { int slot; float score; };
struct KfQuery {
    int64_t id = 0;
    int min_common = 0;
    std::vector<KfMatch> matches;   // lScoreAndMatch
    std::vector<KfDelta> delta;     // state of every entry the query touched, as the query left it
};
}  // namespace

struct orbx_kfdb {
    orbx_handle *h = nullptr;
    bool host_only = true, fma_mode = true;
    int dev = 0, scoring = 0;
    std::vector<KfEntry> ent;                     // indexed by slot
    std::vector<int> free_slots;
    std::unordered_map<int64_t, int> by_id;
    std::unordered_map<uint32_t, std::vector<int>> inv;   // mvInvertedFile: slots per word, in add order
    uint64_t next_seq = 0;
    // st_final: after every query issued; st_view: as of the last query orbx_kfdb_select_groups was called for
    std::vector<KfState> st_final, st_view;
    int form = 0;                                 // of the last query call: 0 reloc, 1 loop
    float min_score = 0.0f;
    std::vector<KfQuery> last;
    size_t next_select = 0;
    std::vector<uint32_t> stamp;                  // host path: touched-in-this-query marks
    uint32_t stamp_now = 0;
    // device side: pooled vectors, one (offset, length) per slot; adds are staged and uploaded by the next query
    std::vector<uint2> slots;
    bool slots_dirty = false;
    std::vector<uint32_t> stage_w;
    std::vector<double> stage_v;
    size_t pool_used = 0, pool_uploaded = 0, pool_cap = 0, garbage = 0;
    uint32_t *d_pool_w = nullptr;
    double *d_pool_v = nullptr;
    DBuf<uint2> d_slots;
    DBuf<uint32_t> d_qw, d_list;
    DBuf<double> d_qv, d_out;
    DBuf<int> d_qbegin, d_qmax;                   // d_qmax[nq] followed by the record cursor
    DBuf<uint8_t> d_conn;
    DBuf<DKfRec> d_rec;
    DKfRec *rec = nullptr;                        // page-locked: the sharer records come back by DMA
    size_t rec_cap = 0;
};

namespace {
hipStream_t kf_stream(orbx_kfdb *db) { return (hipStream_t)orbx_get_stream(db->h); }

bool use_device(const orbx_kfdb *db) {
    if (db->host_only) return false;
    const char *e = getenv("ORBX_KFDB");   // read per call: host | device (default)
    return !(e && strcmp(e, "host") == 0);
}

void apply_delta(std::vector<KfState> &st, int form, const KfDelta &d) {
    KfState &s = st[d.slot];
    s.mark[form] = d.mark; s.words[form] = d.words; s.score[form] = d.score; s.valid[form] = d.valid;
}
// ends the batch of the last query call: the queries whose groups were not selected still leave their state behind
void fold_pending(orbx_kfdb *db) {
    for (size_t q = db->next_select; q < db->last.size(); ++q)
        for (const KfDelta &d : db->last[q].delta)
            if (db->ent[d.slot].live) apply_delta(db->st_view, db->form, d);
    db->next_select = db->last.size();
}

// repack the pool from the host copies (after enough erased words have piled up, or to grow it)
orbx_status pool_rebuild(orbx_kfdb *db, size_t want_cap) {
    hipStream_t s = kf_stream(db);
    HIPCHK(hipStreamSynchronize(s));
    if (want_cap > db->pool_cap) {
        if (db->d_pool_w) hipFree(db->d_pool_w);
        if (db->d_pool_v) hipFree(db->d_pool_v);
        db->d_pool_w = nullptr; db->d_pool_v = nullptr; db->pool_cap = 0;
        HIPCHK(hipMalloc((void **)&db->d_pool_w, want_cap * sizeof(uint32_t)));
        HIPCHK(hipMalloc((void **)&db->d_pool_v, want_cap * sizeof(double)));
        db->pool_cap = want_cap;
    }
    db->stage_w.clear(); db->stage_v.clear();
    size_t off = 0;
    for (size_t i = 0; i < db->ent.size(); ++i) {
        const KfEntry &e = db->ent[i];
        if (!e.live) { db->slots[i] = make_uint2(0, 0); continue; }
        db->slots[i] = make_uint2((uint32_t)off, (uint32_t)e.w.size());
        db->stage_w.insert(db->stage_w.end(), e.w.begin(), e.w.end());
        db->stage_v.insert(db->stage_v.end(), e.v.begin(), e.v.end());
        off += e.w.size();
    }
    db->pool_used = off; db->pool_uploaded = 0; db->garbage = 0; db->slots_dirty = true;
    return ORBX_OK;
}
// uploads what add / erase staged since the last query: one copy per pool array for all new vectors, one for the slot table
orbx_status pool_flush(orbx_kfdb *db) {
    hipStream_t s = kf_stream(db);
    if (db->pool_used > db->pool_cap || db->garbage > std::max<size_t>(1u << 20, db->pool_used / 2)) {
        size_t live = db->pool_used - db->garbage;
        size_t want = db->pool_cap;
        if (live > want || want == 0) want = std::max<size_t>(live + live / 2, 1u << 16);
        if (want >= (1ull << 31)) return orbx_fail(ORBX_CAPACITY, "keyframe database: more than 2^31 pooled words");
        orbx_status st = pool_rebuild(db, want);
        if (st != ORBX_OK) return st;
    }
    const size_t n = db->pool_used - db->pool_uploaded;
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(db->d_pool_w + db->pool_uploaded, db->stage_w.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(db->d_pool_v + db->pool_uploaded, db->stage_v.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
    }
    if (db->slots_dirty && !db->slots.empty()) {
        HIPCHK(db->d_slots.need(db->slots.size()));
        HIPCHK(hipMemcpyAsync(db->d_slots.p, db->slots.data(), db->slots.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
    }
    if (n > 0 || db->slots_dirty) HIPCHK(hipStreamSynchronize(s));   // the staging vectors are pageable and reused
    db->stage_w.clear(); db->stage_v.clear();
    db->pool_uploaded = db->pool_used;
    db->slots_dirty = false;
    return ORBX_OK;
}

int min_common_words(int max_common) { return (int)((float)max_common * 0.8f); }   // `int minCommonWords = maxCommonWords * 0.8f`

// steps 2-3 on the list of step 1, shared by both paths.  words_of(slot) = mn*Words; score_of(k, slot) = the score of list[k]
template <class S> void threshold_and_score(orbx_kfdb *db, KfQuery &Q, const std::vector<int> &list, S &&score_of) {
    const int f = db->form;
    if (list.empty()) return;
    int max_common = 0;
    for (int slot : list) max_common = std::max(max_common, db->st_final[slot].words[f]);
    Q.min_common = min_common_words(max_common);
    for (size_t k = 0; k < list.size(); ++k) {
        const int slot = list[k];
        KfState &S2 = db->st_final[slot];
        if (S2.words[f] > Q.min_common) {
            const float si = score_of(k, slot);
            S2.score[f] = si; S2.valid[f] = 1;
            if (f == 0 || si >= db->min_score) Q.matches.push_back({slot, si});
        }
    }
}
void record_delta(orbx_kfdb *db, KfQuery &Q, int slot) {
    const KfState &s = db->st_final[slot];
    const int f = db->form;
    Q.delta.push_back({slot, s.mark[f], s.words[f], s.score[f], s.valid[f]});
}

// one query, the way the reference runs it: the inverted-file walk
void host_query(orbx_kfdb *db, KfQuery &Q, const uint32_t *qw, const double *qv, int nq, const std::vector<uint8_t> *connected) {
    const int f = db->form;
    std::vector<int> list, touched;
    if (db->stamp.size() < db->ent.size()) db->stamp.resize(db->ent.size(), 0);
    if (++db->stamp_now == 0) { std::fill(db->stamp.begin(), db->stamp.end(), 0); db->stamp_now = 1; }
    for (int i = 0; i < nq; ++i) {
        auto it = db->inv.find(qw[i]);
        if (it == db->inv.end()) continue;
        for (int slot : it->second) {
            KfState &s = db->st_final[slot];
            if (s.mark[f] != Q.id) {
                s.words[f] = 0;
                if (!(connected && (*connected)[slot])) { s.mark[f] = Q.id; list.push_back(slot); }
            }
            s.words[f]++;
            if (db->stamp[slot] != db->stamp_now) { db->stamp[slot] = db->stamp_now; touched.push_back(slot); }
        }
    }
    threshold_and_score(db, Q, list, [&](size_t, int slot) {
        const KfEntry &e = db->ent[slot];
        return (float)bow_score(db->scoring, db->fma_mode, qw, qv, nq, e.w.data(), e.v.data(), (int)e.w.size());
    });
    for (int slot : touched) record_delta(db, Q, slot);
}

// queries [0, nq) of one call on the device; no entry carries the mark of any of them (checked by the caller)
orbx_status device_queries(orbx_kfdb *db, int nq, const int32_t *q_begin, const uint32_t *qw, const double *qv,
                           const std::vector<uint8_t> *connected) {
    orbx_status st = pool_flush(db);
    if (st != ORBX_OK) return st;
    const int nslots = (int)db->slots.size();
    size_t nlive = db->by_id.size();
    if (nlive == 0 || q_begin[nq] == 0) return ORBX_OK;
    hipStream_t s = kf_stream(db);
    const size_t total = (size_t)q_begin[nq];
    HIPCHK(db->d_qw.need(total)); HIPCHK(db->d_qv.need(total)); HIPCHK(db->d_qbegin.need((size_t)nq + 1));
    HIPCHK(hipMemcpyAsync(db->d_qw.p, qw, total * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(db->d_qv.p, qv, total * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(db->d_qbegin.p, q_begin, ((size_t)nq + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (connected) {
        HIPCHK(db->d_conn.need((size_t)nslots));
        HIPCHK(hipMemcpyAsync(db->d_conn.p, connected->data(), (size_t)nslots, hipMemcpyHostToDevice, s));
    }
    // the records of a launch set are bounded by its (query, live entry) pairs: a call whose pairs exceed the budget runs in
    // several sets of whole queries (one round trip each)
    const size_t budget = 8u << 20;
    int chunk = (int)std::min<size_t>(std::max<size_t>(1, budget / nlive), 32768);
    HIPCHK(db->d_qmax.need((size_t)nq + 1));
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int qc = std::min(chunk, nq - q0);
        const size_t cap = (size_t)qc * nlive;
        HIPCHK(db->d_rec.need(cap));
        int *d_qmax = db->d_qmax.p;
        uint32_t *d_cursor = (uint32_t *)(db->d_qmax.p + nq);
        HIPCHK(hipMemsetAsync(d_qmax, 0, ((size_t)nq + 1) * sizeof(int), s));
        orbx_launch_kfdb_common(s, db->d_slots.p, nslots, db->d_pool_w, db->d_qw.p, db->d_qbegin.p, q0, qc,
                                connected ? db->d_conn.p : nullptr, d_qmax, d_cursor, db->d_rec.p, (uint32_t)cap);
        orbx_launch_kfdb_score(s, db->d_rec.p, d_cursor, (uint32_t)cap, d_qmax, db->d_slots.p, db->d_pool_w, db->d_pool_v,
                               db->d_qw.p, db->d_qv.p, db->d_qbegin.p, db->scoring, db->fma_mode ? 1 : 0);
        HIPCHK(hipGetLastError());
        uint32_t nrec = 0;
        HIPCHK(hipMemcpyAsync(&nrec, d_cursor, sizeof(nrec), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (nrec > cap) return orbx_fail(ORBX_HIP_ERROR, "keyframe database: more sharer records than (query, entry) pairs");
        if (nrec > db->rec_cap) {
            if (db->rec) hipHostFree(db->rec);
            db->rec = nullptr; db->rec_cap = 0;
            const size_t c = (size_t)nrec + nrec / 2 + 1024;
            HIPCHK(hipHostMalloc((void **)&db->rec, c * sizeof(DKfRec), hipHostMallocDefault));
            db->rec_cap = c;
        }
        if (nrec) {
            HIPCHK(hipMemcpyAsync(db->rec, db->d_rec.p, (size_t)nrec * sizeof(DKfRec), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        const DKfRec *recs = db->rec;
        // Bucket the records by query (they arrive in no order).  The order of lKFsSharingWords = first encounter = (smallest
        // common word, add order) is observable only through lScoreAndMatch, so only the scored records are sorted; marks,
        // counts and the maximum do not depend on it.
        const int f = db->form;
        std::vector<uint32_t> qoff((size_t)qc + 1, 0), order(nrec);
        for (uint32_t r = 0; r < nrec; ++r) {
            const DKfRec &R = recs[r];
            if (R.q < (uint32_t)q0 || R.q >= (uint32_t)(q0 + qc) || R.slot >= (uint32_t)nslots || !db->ent[R.slot].live)
                return orbx_fail(ORBX_HIP_ERROR, "keyframe database: bad record");
            qoff[R.q - q0 + 1]++;
        }
        for (int q = 0; q < qc; ++q) qoff[q + 1] += qoff[q];
        {
            std::vector<uint32_t> fill(qoff.begin(), qoff.end() - 1);
            for (uint32_t r = 0; r < nrec; ++r) order[fill[recs[r].q - q0]++] = r;
        }
        std::vector<const DKfRec *> scored;
        for (int q = q0; q < q0 + qc; ++q) {
            KfQuery &Q = db->last[q];
            const uint32_t *o = order.data() + qoff[q - q0];
            const uint32_t n = qoff[q - q0 + 1] - qoff[q - q0];
            int max_common = 0;
            bool any = false;
            for (uint32_t k = 0; k < n; ++k) {
                const DKfRec &R = recs[o[k]];
                KfState &S2 = db->st_final[R.slot];
                if (R.flags & ORBX_KF_CONNECTED) { S2.words[f] = 1; continue; }   // reset and incremented at every encounter
                S2.mark[f] = Q.id; S2.words[f] = (int32_t)R.count;
                max_common = std::max(max_common, (int)R.count);
                any = true;
            }
            if (any) {
                Q.min_common = min_common_words(max_common);
                scored.clear();
                for (uint32_t k = 0; k < n; ++k) {
                    const DKfRec &R = recs[o[k]];
                    if ((R.flags & ORBX_KF_CONNECTED) || (int)R.count <= Q.min_common) continue;
                    if (!(R.flags & ORBX_KF_SCORED))
                        return orbx_fail(ORBX_HIP_ERROR, "keyframe database: an entry above the word threshold was not scored");
                    scored.push_back(&R);
                }
                std::sort(scored.begin(), scored.end(), [&](const DKfRec *a, const DKfRec *b) {
                    if (a->minword != b->minword) return a->minword < b->minword;
                    return db->ent[a->slot].seq < db->ent[b->slot].seq;
                });
                for (const DKfRec *R : scored) {
                    KfState &S2 = db->st_final[R->slot];
                    S2.score[f] = R->score; S2.valid[f] = 1;
                    if (f == 0 || R->score >= db->min_score) Q.matches.push_back({(int)R->slot, R->score});
                }
            }
            Q.delta.reserve(n);
            for (uint32_t k = 0; k < n; ++k) record_delta(db, Q, (int)recs[o[k]].slot);
        }
    }
    return ORBX_OK;
}

orbx_status run_queries(orbx_kfdb *db, int form, int nq, const int64_t *ids, const int32_t *q_begin, const uint32_t *qw,
                        const double *qv, const std::vector<uint8_t> *connected, float min_score, int32_t *n_matches,
                        int32_t *min_common) {
    fold_pending(db);
    db->form = form; db->min_score = min_score;
    db->last.assign((size_t)nq, KfQuery());
    db->next_select = 0;
    for (int q = 0; q < nq; ++q) db->last[q].id = ids[q];
    bool device = use_device(db);
    if (device) {
        // An entry whose mark already equals the query id is not re-listed and its count continues (a repeated id, or id 0
        // against fresh entries): that depends on the order of the calls, so such a call takes the reference's walk.
        std::unordered_set<int64_t> qids(ids, ids + nq);
        if ((int)qids.size() != nq) device = false;
        const int64_t lo = *std::min_element(ids, ids + nq), hi = *std::max_element(ids, ids + nq);
        for (size_t i = 0; device && i < db->ent.size(); ++i) {
            const int64_t m = db->st_final[i].mark[form];   // marks are older ids as a rule: the range test settles most
            if (m >= lo && m <= hi && db->ent[i].live && qids.count(m)) device = false;
        }
    }
    if (device) {
        orbx_status st = device_queries(db, nq, q_begin, qw, qv, connected);
        if (st != ORBX_OK) { db->last.clear(); db->st_final = db->st_view; return st; }
    } else {
        for (int q = 0; q < nq; ++q)
            host_query(db, db->last[q], qw + q_begin[q], qv + q_begin[q], q_begin[q + 1] - q_begin[q], connected);
    }
    for (int q = 0; q < nq; ++q) {
        if (n_matches) n_matches[q] = (int32_t)db->last[q].matches.size();
        if (min_common) min_common[q] = db->last[q].min_common;
    }
    return ORBX_OK;
}
}  // namespace

extern "C" orbx_status orbx_bow_score(const orbx_handle *h, int scoring, const uint32_t *a_word, const double *a_value, int na,
                                      const uint32_t *b_word, const double *b_value, int nb, double *score) {
    if (!h || !score || scoring < 0 || scoring > 5) return orbx_fail(ORBX_BAD_ARGUMENT, "orbx_bow_score: null argument or scoring type");
    if (!bow_ok(a_word, a_value, na) || !bow_ok(b_word, b_value, nb)) return orbx_fail(ORBX_BAD_ARGUMENT, "BowVector words must ascend");
    *score = bow_score(scoring, h->p.fp_mode == ORBX_FP_GCC_FMA, a_word, a_value, na, b_word, b_value, nb);
    return ORBX_OK;
}

extern "C" orbx_status orbx_kfdb_create(orbx_handle *h, int scoring, orbx_kfdb **out) {
    if (!h || !out) return orbx_fail(ORBX_BAD_ARGUMENT, "null argument");
    *out = nullptr;
    if (scoring < 0 || scoring > 5) return orbx_fail(ORBX_BAD_ARGUMENT, "scoring type out of range [0,5]");
    orbx_kfdb *db = new orbx_kfdb();
    db->h = h; db->scoring = scoring;
    db->host_only = h->host_only;
    db->dev = h->dev;
    db->fma_mode = h->p.fp_mode == ORBX_FP_GCC_FMA;
    *out = db;
    return ORBX_OK;
}

static void kfdb_release_device(orbx_kfdb *db) {
    if (db->host_only) return;
    hipSetDevice(db->dev);
    hipStreamSynchronize(kf_stream(db));
    if (db->d_pool_w) hipFree(db->d_pool_w);
    if (db->d_pool_v) hipFree(db->d_pool_v);
    db->d_pool_w = nullptr; db->d_pool_v = nullptr; db->pool_cap = 0;
    db->d_slots.release(); db->d_qw.release(); db->d_list.release(); db->d_qv.release(); db->d_out.release();
    db->d_qbegin.release(); db->d_qmax.release(); db->d_conn.release(); db->d_rec.release();
    if (db->rec) hipHostFree(db->rec);
    db->rec = nullptr; db->rec_cap = 0;
}

extern "C" void orbx_kfdb_destroy(orbx_kfdb *db) {
    if (!db) return;
    kfdb_release_device(db);
    delete db;
}

extern "C" orbx_status orbx_kfdb_clear(orbx_kfdb *db) {
    if (!db) return orbx_fail(ORBX_BAD_ARGUMENT, "null database");
    db->ent.clear(); db->free_slots.clear(); db->by_id.clear(); db->inv.clear();
    db->st_final.clear(); db->st_view.clear(); db->last.clear(); db->next_select = 0; db->stamp.clear();
    db->slots.clear(); db->slots_dirty = false; db->stage_w.clear(); db->stage_v.clear();
    db->pool_used = db->pool_uploaded = db->garbage = 0;
    return ORBX_OK;
}

extern "C" int orbx_kfdb_size(const orbx_kfdb *db) { return db ? (int)db->by_id.size() : 0; }

extern "C" orbx_status orbx_kfdb_add(orbx_kfdb *db, int64_t id, const uint32_t *bow_word, const double *bow_value, int n) {
    if (!db) return orbx_fail(ORBX_BAD_ARGUMENT, "null database");
    if (!bow_ok(bow_word, bow_value, n)) return orbx_fail(ORBX_BAD_ARGUMENT, "BowVector words must ascend");
    if (db->by_id.count(id)) return orbx_fail(ORBX_BAD_ARGUMENT, "keyframe id is already in the database");
    if (db->pool_used + (size_t)n >= (1ull << 31)) return orbx_fail(ORBX_CAPACITY, "keyframe database: more than 2^31 pooled words");
    fold_pending(db);
    db->last.clear(); db->next_select = 0;   // the results of the last query call name entries by slot
    int slot;
    if (!db->free_slots.empty()) { slot = db->free_slots.back(); db->free_slots.pop_back(); }
    else {
        slot = (int)db->ent.size();
        db->ent.emplace_back(); db->st_final.emplace_back(); db->st_view.emplace_back(); db->slots.push_back(make_uint2(0, 0));
    }
    KfEntry &e = db->ent[slot];
    e.id = id; e.seq = db->next_seq++; e.live = true;
    e.w.assign(bow_word, bow_word + n); e.v.assign(bow_value, bow_value + n);
    db->st_final[slot] = KfState(); db->st_view[slot] = KfState();
    db->by_id[id] = slot;
    for (int i = 0; i < n; ++i) db->inv[bow_word[i]].push_back(slot);
    if (!db->host_only) {
        db->slots[slot] = make_uint2((uint32_t)db->pool_used, (uint32_t)n);
        db->stage_w.insert(db->stage_w.end(), bow_word, bow_word + n);
        db->stage_v.insert(db->stage_v.end(), bow_value, bow_value + n);
        db->pool_used += (size_t)n;
        db->slots_dirty = true;
    }
    return ORBX_OK;
}

extern "C" orbx_status orbx_kfdb_erase(orbx_kfdb *db, int64_t id) {
    if (!db) return orbx_fail(ORBX_BAD_ARGUMENT, "null database");
    auto it = db->by_id.find(id);
    if (it == db->by_id.end()) return orbx_fail(ORBX_BAD_ARGUMENT, "keyframe id is not in the database");
    fold_pending(db);
    db->last.clear(); db->next_select = 0;
    const int slot = it->second;
    KfEntry &e = db->ent[slot];
    for (uint32_t w : e.w) {   // the other entries of every list keep their order
        auto li = db->inv.find(w);
        if (li == db->inv.end()) continue;
        auto &l = li->second;
        auto p = std::find(l.begin(), l.end(), slot);
        if (p != l.end()) l.erase(p);
        if (l.empty()) db->inv.erase(li);
    }
    if (!db->host_only) {
        db->garbage += e.w.size();
        db->slots[slot] = make_uint2(0, 0);
        db->slots_dirty = true;
    }
    e.live = false; e.w.clear(); e.w.shrink_to_fit(); e.v.clear(); e.v.shrink_to_fit();
    db->by_id.erase(it);
    db->free_slots.push_back(slot);
    return ORBX_OK;
}

extern "C" orbx_status orbx_kfdb_score_entries(orbx_kfdb *db, const uint32_t *q_word, const double *q_value, int nq,
                                               const int64_t *ids, int n, double *scores) {
    if (!db || n < 0 || (n > 0 && (!ids || !scores))) return orbx_fail(ORBX_BAD_ARGUMENT, "null argument");
    if (!bow_ok(q_word, q_value, nq)) return orbx_fail(ORBX_BAD_ARGUMENT, "BowVector words must ascend");
    std::vector<uint32_t> list((size_t)n);
    for (int i = 0; i < n; ++i) {
        auto it = db->by_id.find(ids[i]);
        if (it == db->by_id.end()) return orbx_fail(ORBX_BAD_ARGUMENT, "keyframe id is not in the database");
        list[i] = (uint32_t)it->second;
    }
    if (n == 0) return ORBX_OK;
    if (!use_device(db)) {
        for (int i = 0; i < n; ++i) {
            const KfEntry &e = db->ent[list[i]];
            scores[i] = bow_score(db->scoring, db->fma_mode, q_word, q_value, nq, e.w.data(), e.v.data(), (int)e.w.size());
        }
        return ORBX_OK;
    }
    if (db->scoring == 3) return orbx_fail(ORBX_UNSUPPORTED, "KL scoring needs libm's log: use orbx_bow_score or ORBX_KFDB=host");
    HIPCHK(hipSetDevice(db->dev));
    orbx_status st = pool_flush(db);
    if (st != ORBX_OK) return st;
    hipStream_t s = kf_stream(db);
    HIPCHK(db->d_qw.need((size_t)nq + 1)); HIPCHK(db->d_qv.need((size_t)nq + 1));
    HIPCHK(db->d_list.need((size_t)n)); HIPCHK(db->d_out.need((size_t)n));
    if (nq > 0) {
        HIPCHK(hipMemcpyAsync(db->d_qw.p, q_word, (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(db->d_qv.p, q_value, (size_t)nq * sizeof(double), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(db->d_list.p, list.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    orbx_launch_kfdb_score_slots(s, db->d_list.p, n, db->d_slots.p, db->d_pool_w, db->d_pool_v, db->d_qw.p, db->d_qv.p, nq,
                                 db->scoring, db->fma_mode ? 1 : 0, db->d_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(scores, db->d_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ORBX_OK;
}

static orbx_status check_queries(orbx_kfdb *db, int nq, const int64_t *ids, const int32_t *q_begin, const uint32_t *qw,
                                 const double *qv) {
    if (!db || nq < 0 || (nq > 0 && (!ids || !q_begin))) return orbx_fail(ORBX_BAD_ARGUMENT, "null argument");
    if (nq > 0 && q_begin[0] != 0) return orbx_fail(ORBX_BAD_ARGUMENT, "q_begin[0] != 0");
    for (int q = 0; q < nq; ++q) {
        if (q_begin[q + 1] < q_begin[q]) return orbx_fail(ORBX_BAD_ARGUMENT, "q_begin must not decrease");
        if (!bow_ok(qw ? qw + q_begin[q] : nullptr, qv ? qv + q_begin[q] : nullptr, q_begin[q + 1] - q_begin[q]))
            return orbx_fail(ORBX_BAD_ARGUMENT, "BowVector words must ascend");
    }
    if (db->scoring == 3 && use_device(db))
        return orbx_fail(ORBX_UNSUPPORTED, "KL scoring needs libm's log: use a host-only handle or ORBX_KFDB=host");
    if (!db->host_only) HIPCHK(hipSetDevice(db->dev));
    return ORBX_OK;
}

extern "C" orbx_status orbx_kfdb_query_reloc(orbx_kfdb *db, int nqueries, const int64_t *query_ids, const int32_t *q_begin,
                                             const uint32_t *q_word, const double *q_value, int32_t *n_matches,
                                             int32_t *min_common_words) {
    orbx_status st = check_queries(db, nqueries, query_ids, q_begin, q_word, q_value);
    if (st != ORBX_OK) return st;
    return run_queries(db, 0, nqueries, query_ids, q_begin, q_word, q_value, nullptr, 0.0f, n_matches, min_common_words);
}

extern "C" orbx_status orbx_kfdb_query_loop(orbx_kfdb *db, int64_t query_id, const uint32_t *q_word, const double *q_value, int nq,
                                            const int64_t *connected_ids, int nconnected, float min_score, int32_t *n_matches,
                                            int32_t *min_common_words) {
    if (nq < 0 || nconnected < 0 || (nconnected > 0 && !connected_ids)) return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    const int32_t q_begin[2] = {0, nq};
    orbx_status st = check_queries(db, 1, &query_id, q_begin, q_word, q_value);
    if (st != ORBX_OK) return st;
    std::vector<uint8_t> connected(db->ent.size(), 0);   // spConnectedKeyFrames; keyframes outside the database cannot be met
    for (int i = 0; i < nconnected; ++i) {
        auto it = db->by_id.find(connected_ids[i]);
        if (it != db->by_id.end()) connected[it->second] = 1;
    }
    return run_queries(db, 1, 1, &query_id, q_begin, q_word, q_value, &connected, min_score, n_matches, min_common_words);
}

extern "C" orbx_status orbx_kfdb_query_matches(orbx_kfdb *db, int query, int64_t *ids, float *scores, int cap, int *n) {
    if (!db || !n || query < 0 || (size_t)query >= db->last.size()) return orbx_fail(ORBX_BAD_ARGUMENT, "no such query in the last call");
    const KfQuery &Q = db->last[query];
    *n = (int)Q.matches.size();
    if (*n > cap) return orbx_fail(ORBX_CAPACITY, "lScoreAndMatch is longer than the caller's buffers");
    for (int i = 0; i < *n; ++i) {
        if (ids) ids[i] = db->ent[Q.matches[i].slot].id;
        if (scores) scores[i] = Q.matches[i].score;
    }
    return ORBX_OK;
}

extern "C" orbx_status orbx_kfdb_query_touched(orbx_kfdb *db, int query, int64_t *ids, int cap, int *n) {
    if (!db || !n || query < 0 || (size_t)query >= db->last.size()) return orbx_fail(ORBX_BAD_ARGUMENT, "no such query in the last call");
    const KfQuery &Q = db->last[query];
    *n = (int)Q.delta.size();
    if (*n > cap) return orbx_fail(ORBX_CAPACITY, "more touched entries than the caller's buffer holds");
    for (int i = 0; i < *n; ++i) ids[i] = db->ent[Q.delta[i].slot].id;
    return ORBX_OK;
}

extern "C" orbx_status orbx_kfdb_select_groups(orbx_kfdb *db, int query, const int32_t *neigh_begin, const int64_t *neigh_ids,
                                               int64_t *candidates, int cap, int *n, int *n_unscored_reads) {
    if (!db || !n) return orbx_fail(ORBX_BAD_ARGUMENT, "null argument");
    if (query < 0 || (size_t)query >= db->last.size() || (size_t)query != db->next_select)
        return orbx_fail(ORBX_BAD_ARGUMENT, "select_groups runs once per query of the last call, in order, before any other call on the database");
    const KfQuery &Q = db->last[query];
    const int f = db->form, nm = (int)Q.matches.size();
    if (nm > 0 && (!neigh_begin || neigh_begin[0] != 0)) return orbx_fail(ORBX_BAD_ARGUMENT, "neigh_begin");
    for (int i = 0; i < nm; ++i)
        if (neigh_begin[i + 1] < neigh_begin[i] || (neigh_begin[i + 1] > 0 && !neigh_ids)) return orbx_fail(ORBX_BAD_ARGUMENT, "neigh_begin");
    // steps 4-5 see marks, counts and scores as of this query, not as of the end of the batch
    for (const KfDelta &d : Q.delta) apply_delta(db->st_view, f, d);
    db->next_select++;
    *n = 0;
    int unscored = 0;
    if (n_unscored_reads) *n_unscored_reads = 0;
    if (nm == 0) return ORBX_OK;
    std::vector<std::pair<float, int>> acc_and_match;   // lAccScoreAndMatch
    float bestAccScore = f == 1 ? db->min_score : 0.0f;
    for (int i = 0; i < nm; ++i) {
        float bestScore = Q.matches[i].score, accScore = Q.matches[i].score;
        int best = Q.matches[i].slot;
        for (int k = neigh_begin[i]; k < neigh_begin[i + 1]; ++k) {
            auto it = db->by_id.find(neigh_ids[k]);
            if (it == db->by_id.end()) continue;                      // a keyframe outside the database carries no mark
            const KfState &s = db->st_view[it->second];
            if (s.mark[f] != Q.id) continue;
            if (f == 1 && !(s.words[f] > Q.min_common)) continue;     // only the loop form checks the word count (:205)
            // F8: the score may be one an earlier query left, or was never written (read as 0.0f and counted)
            float sc = 0.0f;
            if (s.valid[f]) sc = s.score[f]; else unscored++;
            accScore += sc;
            if (sc > bestScore) { best = it->second; bestScore = sc; }
        }
        acc_and_match.push_back({accScore, best});
        if (accScore > bestAccScore) bestAccScore = accScore;
    }
    const float minScoreToRetain = 0.75f * bestAccScore;
    std::vector<int> out;
    for (auto &am : acc_and_match)
        if (am.first > minScoreToRetain && std::find(out.begin(), out.end(), am.second) == out.end()) out.push_back(am.second);
    *n = (int)out.size();
    if (n_unscored_reads) *n_unscored_reads = unscored;
    if (*n > cap) return orbx_fail(ORBX_CAPACITY, "more candidates than the caller's buffer holds");
    for (int i = 0; i < *n; ++i) candidates[i] = db->ent[out[i]].id;
    return ORBX_OK;
}

extern "C" orbx_status orbx_kfdb_state(orbx_kfdb *db, int64_t id, int loop_form, int64_t *mark, int32_t *words, float *score,
                                       int *score_valid) {
    if (!db || (loop_form != 0 && loop_form != 1)) return orbx_fail(ORBX_BAD_ARGUMENT, "bad argument");
    auto it = db->by_id.find(id);
    if (it == db->by_id.end()) return orbx_fail(ORBX_BAD_ARGUMENT, "keyframe id is not in the database");
    fold_pending(db);
    const KfState &s = db->st_view[it->second];
    if (mark) *mark = s.mark[loop_form];
    if (words) *words = s.words[loop_form];
    if (score) *score = s.score[loop_form];
    if (score_valid) *score_valid = s.valid[loop_form];
    return ORBX_OK;
}
