"""ORB_SLAM2::KeyFrameDatabase behind the C ABI (reference src/KeyFrameDatabase.cc): add / erase / clear, the two
Detect*Candidates queries and plain vocabulary scores.  The BowVectors of the entries live on the extractor's device; the
common-word counts and the scores are HIP kernels (k_kfdb_common, k_kfdb_score), the order-dependent selection and the
per-keyframe marks / counts / scores the reference keeps across queries are folded on the host (include/orbx.h)."""
from __future__ import annotations
import ctypes as C
import numpy as np
from ._capi import check, ptr, lib


def _bow(v):
    w, x = v
    return np.ascontiguousarray(w, np.uint32), np.ascontiguousarray(x, np.float64)


def bow_score(extractor, scoring, a, b):
    """TemplatedVocabulary::score(a, b) on the host, all six scoring types; a, b = (word ids, values)"""
    (aw, av), (bw, bv) = _bow(a), _bow(b)
    s = C.c_double(0)
    check(lib().orbx_bow_score(extractor.handle, int(scoring), ptr(aw), ptr(av), len(aw), ptr(bw), ptr(bv), len(bw), C.byref(s)))
    return s.value


class KeyFrameDatabase:
    def __init__(self, extractor, vocabulary=None, *, scoring=None):
        """scoring: a DBoW2::ScoringType, or taken from `vocabulary` (an ORBVocabulary)"""
        self._ex = extractor
        if scoring is None:
            scoring = lib().orbx_vocabulary_scoring(vocabulary._h) if vocabulary is not None else 0
        self.scoring = int(scoring)
        self._h = C.c_void_p()
        check(lib().orbx_kfdb_create(extractor.handle, self.scoring, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().orbx_kfdb_destroy(self._h)
            except Exception:   # interpreter shutdown: module globals are already gone
                pass
            self._h = None

    def __len__(self):
        return lib().orbx_kfdb_size(self._h)

    def clear(self):
        check(lib().orbx_kfdb_clear(self._h))

    def add(self, kf_id, bow):
        w, v = _bow(bow)
        check(lib().orbx_kfdb_add(self._h, int(kf_id), ptr(w), ptr(v), len(w)))

    def erase(self, kf_id):
        check(lib().orbx_kfdb_erase(self._h, int(kf_id)))

    def score_entries(self, bow, ids):
        """mpVocabulary->score(bow, entry) per named entry (float64)"""
        w, v = _bow(bow)
        ids = np.ascontiguousarray(ids, np.int64)
        out = np.zeros(max(len(ids), 1), np.float64)
        check(lib().orbx_kfdb_score_entries(self._h, ptr(w), ptr(v), len(w), ptr(ids), len(ids), ptr(out)))
        return out[:len(ids)]

    def _matches(self, q, n):
        ids = np.zeros(max(n, 1), np.int64); sc = np.zeros(max(n, 1), np.float32); got = C.c_int(0)
        check(lib().orbx_kfdb_query_matches(self._h, q, ptr(ids), ptr(sc), max(n, 1), C.byref(got)))
        return ids[:got.value], sc[:got.value]

    def query_reloc(self, query_ids, bows):
        """steps 1-3 of DetectRelocalizationCandidates for len(bows) frames as if run in that order; per query
        (ids of lScoreAndMatch in list order, float32 scores, minCommonWords)"""
        Q = len(bows)
        ids = np.ascontiguousarray(query_ids, np.int64)
        assert len(ids) == Q
        vs = [_bow(b) for b in bows]
        begin = np.zeros(Q + 1, np.int32)
        begin[1:] = np.cumsum([len(w) for w, _ in vs])
        w = np.concatenate([x for x, _ in vs] + [np.zeros(1, np.uint32)])
        v = np.concatenate([x for _, x in vs] + [np.zeros(1, np.float64)])
        nm = np.zeros(max(Q, 1), np.int32); mc = np.zeros(max(Q, 1), np.int32)
        check(lib().orbx_kfdb_query_reloc(self._h, Q, ptr(ids), ptr(begin), ptr(w), ptr(v), ptr(nm), ptr(mc)))
        return [self._matches(q, int(nm[q])) + (int(mc[q]),) for q in range(Q)]

    def query_loop(self, query_id, bow, connected_ids, min_score):
        w, v = _bow(bow)
        conn = np.ascontiguousarray(connected_ids, np.int64)
        nm = np.zeros(1, np.int32); mc = np.zeros(1, np.int32)
        check(lib().orbx_kfdb_query_loop(self._h, int(query_id), ptr(w), ptr(v), len(w), ptr(conn), len(conn),
                                         float(min_score), ptr(nm), ptr(mc)))
        return self._matches(0, int(nm[0])) + (int(mc[0]),)

    def touched(self, query=0):
        got = C.c_int(0)
        lib().orbx_kfdb_query_touched(self._h, query, None, 0, C.byref(got))
        ids = np.zeros(max(got.value, 1), np.int64)
        check(lib().orbx_kfdb_query_touched(self._h, query, ptr(ids), max(got.value, 1), C.byref(got)))
        return ids[:got.value]

    def select_groups(self, query, neighbours):
        """steps 4-5 for query `query` of the last query call; neighbours[i] = ids of GetBestCovisibilityKeyFrames(10) of
        lScoreAndMatch[i].  Returns (candidate ids in order, number of reads of a never-written score)."""
        begin = np.zeros(len(neighbours) + 1, np.int32)
        begin[1:] = np.cumsum([len(x) for x in neighbours])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int64) for x in neighbours] + [np.zeros(1, np.int64)]))
        out = np.zeros(max(len(neighbours), 1), np.int64); n = C.c_int(0); nu = C.c_int(0)
        check(lib().orbx_kfdb_select_groups(self._h, int(query), ptr(begin), ptr(flat), ptr(out), len(out), C.byref(n), C.byref(nu)))
        return out[:n.value].copy(), nu.value

    def state(self, kf_id, loop=False):
        """(mark, words, score, score_valid) of the relocalisation (loop=False) or loop form"""
        m = C.c_int64(0); w = C.c_int(0); s = C.c_float(0); ok = C.c_int(0)
        check(lib().orbx_kfdb_state(self._h, int(kf_id), int(bool(loop)), C.byref(m), C.byref(w), C.byref(s), C.byref(ok)))
        return m.value, w.value, np.float32(s.value), ok.value
