"""Loader and adapter for the compiled reference (oracle/ref/: the reference's own DBoW2 and KeyFrameDatabase sources behind
stand-ins for cv::Mat, KeyFrame and Frame, built by oracle/ref/build_ref.py into oracle/_ref/ under two flag sets).

    Ref(fp_mode)            one of the two libraries: FP_STRICT -> -O3 -ffp-contract=off, FP_GCC_FMA -> -O3 -mfma
    write_vocabulary        a tests/test_bow_transform.py tree in the loadFromTextFile format
    write_flat_vocabulary   a root with `nwords` leaf children: mpVoc->size() covers every word id of a kfdb_driver.World
    Tee                     plays the calls kfdb_driver.Checked makes on a library database on the compiled
                            KeyFrameDatabase as well, compares the two directly, and hands the REFERENCE's candidates, marks,
                            word counts and scores back to Checked, which compares them with the model

Nothing here reads the reference tree; only available() asks whether it exists, to word the skip reason."""
import ctypes as C
import importlib.util
import os
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FP_GCC_FMA, FP_STRICT = 0, 1

_spec = importlib.util.spec_from_file_location("orbx_build_ref", os.path.join(ROOT, "oracle", "ref", "build_ref.py"))
build_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(build_ref)

SKIP_REASON = ("the compiled reference is absent (oracle/_ref/ holds no libraries) AND the reference tree it is built from is "
               "absent (%s): nothing to compare with" % build_ref.reference_dir())


def available():
    """True when the two libraries exist, building them when only the reference tree does"""
    if build_ref.reference_present():
        build_ref.build()
    return build_ref.built()


def cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("flags"):
                    return " fma " in line + " "
    except OSError:
        pass
    return False


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bow(v):
    return np.ascontiguousarray(v[0], np.uint32), np.ascontiguousarray(v[1], np.float64)


_LIBS = {}
_TMP = None


def tmpdir():
    global _TMP
    if _TMP is None:
        _TMP = tempfile.TemporaryDirectory(prefix="ref_dbow2_")
    return _TMP.name


class Ref:
    """one compiled library; Ref(fp_mode) is cached per mode"""

    def __new__(cls, fp_mode):
        if fp_mode not in _LIBS:
            self = object.__new__(cls)
            self._load(fp_mode)
            _LIBS[fp_mode] = self
        return _LIBS[fp_mode]

    def _load(self, fp_mode):
        variant = {FP_GCC_FMA: "fma", FP_STRICT: "strict"}[fp_mode]
        if variant == "fma" and not cpu_has_fma():
            raise RuntimeError("oracle/_ref/libref_dbow2_fma.so is built with -mfma and this CPU does not list `fma` in /proc/cpuinfo")
        self.fp_mode, self.variant = fp_mode, variant
        L = self.L = C.CDLL(build_ref.lib_path(variant))
        vp, ci, i64 = C.c_void_p, C.c_int, C.c_int64
        L.ref_error.restype = C.c_char_p
        L.ref_compiler.restype = C.c_char_p
        L.ref_voc_load.argtypes = [C.c_char_p, vp]
        L.ref_voc_free.argtypes = [vp]; L.ref_voc_free.restype = None
        for f in (L.ref_voc_size, L.ref_voc_scoring, L.ref_voc_weighting):
            f.argtypes = [vp]
        L.ref_voc_transform.argtypes = [vp, vp, ci, ci] + [vp] * 10
        L.ref_voc_score.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp]
        L.ref_bow_normalize.argtypes = [vp, vp, ci, ci]
        L.ref_db_create.argtypes = [vp, vp]
        L.ref_db_free.argtypes = [vp]; L.ref_db_free.restype = None
        L.ref_kf_new.argtypes = [vp, i64, vp, vp, ci]
        L.ref_db_add.argtypes = [vp, ci]; L.ref_db_erase.argtypes = [vp, ci]; L.ref_db_clear.argtypes = [vp]
        L.ref_kf_set_connected.argtypes = [vp, ci, vp, ci]
        L.ref_kf_set_ordered.argtypes = [vp, ci, vp, vp, vp]
        L.ref_db_detect_loop.argtypes = [vp, ci, C.c_float, vp, ci, vp]
        L.ref_db_detect_reloc.argtypes = [vp, i64, vp, vp, ci, vp, ci, vp]
        L.ref_kf_fields.argtypes = [vp, ci, vp, vp, vp]
        assert L.ref_fp_fast_fma() == (variant == "fma")
        self._flat = {}

    def ck(self, rc):
        assert rc == 0, self.L.ref_error().decode()

    def vocabulary(self, path):
        return RefVocabulary(self, path)

    def flat_vocabulary(self, nwords, scoring=0):
        """cached: a root with nwords leaf children, weighting TF_IDF"""
        key = (int(nwords), int(scoring))
        if key not in self._flat:
            path = os.path.join(tmpdir(), "flat_%d_%d.txt" % key)
            if not os.path.exists(path):
                write_flat_vocabulary(path, nwords, scoring)
            self._flat[key] = RefVocabulary(self, path)
            assert self._flat[key].size() == nwords
        return self._flat[key]

    def normalize(self, bow, norm):
        """BowVector::normalize; norm: 1 = L1, 2 = L2"""
        w, v = _bow(bow)
        v = v.copy()
        self.ck(self.L.ref_bow_normalize(_p(w), _p(v), len(w), {1: 0, 2: 1}[norm]))
        return v

    def score(self, scoring, a, b):
        """TemplatedVocabulary::score of a vocabulary with that scoring type"""
        return self.flat_vocabulary(1, scoring).score(a, b)


class RefVocabulary:
    def __init__(self, ref, path):
        self.ref = ref
        self.h = C.c_void_p()
        ref.ck(ref.L.ref_voc_load(str(path).encode(), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            try:
                self.ref.L.ref_voc_free(self.h)
            except Exception:
                pass
            self.h = None

    def size(self):
        return self.ref.L.ref_voc_size(self.h)

    def scoring(self):
        return self.ref.L.ref_voc_scoring(self.h)

    def weighting(self):
        return self.ref.L.ref_voc_weighting(self.h)

    def score(self, a, b):
        (aw, av), (bw, bv) = _bow(a), _bow(b)
        s = C.c_double(0)
        self.ref.ck(self.ref.L.ref_voc_score(self.h, _p(aw), _p(av), len(aw), _p(bw), _p(bv), len(bw), C.byref(s)))
        return s.value

    def transform(self, desc, levelsup):
        """the layout of oracle.bow_transform: (word_id, weight, node_id, (bow_word, bow_value), (fv_node, fv_begin, fv_index)).
        node_id is 0xFFFFFFFF where the reference assigns none (a leaf above level L - levelsup)."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32); n = len(d)
        wid = np.zeros(max(n, 1), np.uint32); w = np.zeros(max(n, 1), np.float64); nid = np.zeros(max(n, 1), np.uint32)
        bw = np.zeros(max(n, 1), np.uint32); bv = np.zeros(max(n, 1), np.float64)
        fn = np.zeros(max(n, 1), np.uint32); fb = np.zeros(n + 2, np.int32); fi = np.zeros(max(n, 1), np.uint32)
        nb, nn = C.c_int(0), C.c_int(0)
        self.ref.ck(self.ref.L.ref_voc_transform(self.h, _p(d), n, int(levelsup), _p(wid), _p(w), _p(nid), _p(bw), _p(bv),
                                                 C.byref(nb), _p(fn), _p(fb), _p(fi), C.byref(nn)))
        return (wid[:n].copy(), w[:n].copy(), nid[:n].copy(), (bw[:nb.value].copy(), bv[:nb.value].copy()),
                (fn[:nn.value].copy(), fb[:nn.value + 1].copy(), fi[:fb[nn.value]].copy()))


# ------------------------------------------------------------------------------------------------ vocabulary files
# loadFromTextFile reads lines `while(!f.eof())`: a newline after the last node would make it read one more, empty, node.
# The files therefore end without one (ORBVocabulary.load_text skips empty lines and reads both forms alike).
def write_vocabulary(path, voc, children):
    """a random_vocabulary() tree (tests/test_bow_transform.py): header `k L scoring weighting`, then the nodes 1.. in id order as
    `parent is_leaf d0 .. d31 weight`; the weight is written with repr(), which strtod reads back to the same double"""
    parent = np.zeros(voc["n_nodes"], np.int64)
    for p, ch in enumerate(children):
        for c in ch:
            parent[c] = p
    lines = ["%d %d %d %d" % (voc["k"], voc["L"], voc["scoring"], voc["weighting"])]
    for i in range(1, voc["n_nodes"]):
        lines.append("%d %d %s %r" % (parent[i], int(not children[i]), " ".join(str(int(b)) for b in voc["desc"][i]),
                                      float(voc["weight"][i])))
    with open(path, "w") as f:
        f.write("\n".join(lines))


def write_flat_vocabulary(path, nwords, scoring):
    lines = ["10 1 %d 0" % scoring] + ["0 1 " + "0 " * 32 + "1.0"] * nwords
    with open(path, "w") as f:
        f.write("\n".join(lines))


# ------------------------------------------------------------------------------------------------ the database adapter
def fbits(x):
    return np.asarray(x, np.float32).view(np.uint32)


class RefDatabase:
    """ORB_SLAM2::KeyFrameDatabase of one compiled library over a flat vocabulary; keyframes are handles"""

    def __init__(self, ref, nwords, scoring=0, voc=None):
        self.ref, self.L = ref, ref.L
        self.voc = ref.flat_vocabulary(nwords, scoring) if voc is None else voc
        assert self.voc.scoring() == scoring
        self.h = C.c_void_p()
        ref.ck(self.L.ref_db_create(self.voc.h, C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            try:
                self.L.ref_db_free(self.h)
            except Exception:
                pass
            self.h = None

    def new_keyframe(self, kf_id, bow):
        w, v = _bow(bow)
        assert len(w) == 0 or int(w.max()) < self.voc.size(), "word id beyond mpVoc->size(): the reference would index past mvInvertedFile"
        k = self.L.ref_kf_new(self.h, int(kf_id), _p(w), _p(v), len(w))
        assert k >= 0, self.L.ref_error().decode()
        return k

    def add(self, k):
        self.ref.ck(self.L.ref_db_add(self.h, k))

    def erase(self, k):
        self.ref.ck(self.L.ref_db_erase(self.h, k))

    def clear(self):
        self.ref.ck(self.L.ref_db_clear(self.h))

    def set_connected(self, k, handles):
        a = np.ascontiguousarray(handles, np.int32)
        self.ref.ck(self.L.ref_kf_set_connected(self.h, k, _p(a), len(a)))

    def set_ordered(self, lists):
        """lists: {handle: [handles, best first]}"""
        kf = np.ascontiguousarray(list(lists), np.int32)
        begin = np.zeros(len(kf) + 1, np.int32)
        begin[1:] = np.cumsum([len(x) for x in lists.values()])
        flat = np.ascontiguousarray([j for x in lists.values() for j in x] + [0], np.int32)
        self.ref.ck(self.L.ref_kf_set_ordered(self.h, len(kf), _p(kf), _p(begin), _p(flat)))

    def _ids(self, call):
        out = np.zeros(8192, np.int64); n = C.c_int(0)
        self.ref.ck(call(_p(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def detect_loop(self, k, min_score):
        return self._ids(lambda *a: self.L.ref_db_detect_loop(self.h, k, C.c_float(float(min_score)), *a))

    def detect_reloc(self, frame_id, bow):
        w, v = _bow(bow)
        assert len(w) == 0 or int(w.max()) < self.voc.size()
        return self._ids(lambda *a: self.L.ref_db_detect_reloc(self.h, int(frame_id), _p(w), _p(v), len(w), *a))

    def fields(self, k, loop):
        """(mark, words, float32 score) of the relocalisation (loop=False) or loop form"""
        m = np.zeros(2, np.int64); n = np.zeros(2, np.int32); s = np.zeros(2, np.float32)
        self.ref.ck(self.L.ref_kf_fields(self.h, k, _p(m), _p(n), _p(s)))
        i = int(bool(loop))
        return int(m[i]), int(n[i]), s[i]


class Tee:
    """the `db` of a kfdb_driver.Checked: every call goes to the library database `lib` (host or device path) AND to the
    compiled KeyFrameDatabase.  The library's answers are compared with the reference's directly, here.  Checked gets the
    reference's candidates (select_groups) and the reference's marks, word counts and scores (state), and compares those with
    the model; lScoreAndMatch, minCommonWords and the count of never-written reads, which the reference does not return,
    are the library's.  The reference keeps covisibility in the KeyFrames: it is copied from the World before every query."""

    def __init__(self, world, lib, ref, voc=None):
        """voc: a RefVocabulary whose size covers every word id; by default a flat one of world.vocab words"""
        self.w, self.lib = world, lib
        self.rdb = RefDatabase(ref, world.vocab, lib.scoring, voc)
        self.handle = {}      # live id -> handle
        self.all = []         # (handle, model KeyFrame) of every keyframe ever added, erased ones included
        self.cands = []
        self.compared = dict(candidates=0, states=0, scores=0, all_states=0)

    # ---- mutations
    def add(self, kf_id, bow):
        self.lib.add(kf_id, bow)
        k = self.rdb.new_keyframe(kf_id, bow)
        self.rdb.add(k)
        self.handle[kf_id] = k
        self.all.append((k, self.w.kfs[kf_id]))

    def erase(self, kf_id):
        self.lib.erase(kf_id)
        self.rdb.erase(self.handle.pop(kf_id))

    def __len__(self):
        return len(self.lib)

    # ---- queries
    def _graph(self):
        self.rdb.set_ordered({self.handle[i]: [self.handle[k.mnId] for k in kf.best_covis] for i, kf in self.w.kfs.items()})

    def query_reloc(self, query_ids, bows):
        got = self.lib.query_reloc(query_ids, bows)
        self._graph()
        self.cands = [self.rdb.detect_reloc(i, b) for i, b in zip(query_ids, bows)]   # one after the other
        return got

    def query_loop(self, query_id, bow, connected_ids, min_score):
        got = self.lib.query_loop(query_id, bow, connected_ids, min_score)
        self._graph()
        cur = self.rdb.new_keyframe(query_id, bow)
        self.rdb.set_connected(cur, [self.handle[i] for i in connected_ids if i in self.handle])
        self.cands = [self.rdb.detect_loop(cur, min_score)]
        return got

    def select_groups(self, query, neighbours):
        cand, unscored = self.lib.select_groups(query, neighbours)
        ref = self.cands[query]
        assert list(cand) == list(ref), ("library against compiled reference", list(cand), list(ref))
        self.compared["candidates"] += 1
        return ref, unscored

    def state(self, kf_id, loop=False):
        m, n, s, ok = self.lib.state(kf_id, loop)
        rm, rn, rs = self.rdb.fields(self.handle[kf_id], loop)
        assert (m, n) == (rm, rn), ("library against compiled reference", kf_id, loop, (m, n), (rm, rn))
        # a score nothing wrote yet: 0.0f in the reference's stand-in KeyFrame (rule F8), flagged invalid in the library
        assert fbits(rs) == (fbits(s) if ok else 0), ("library against compiled reference", kf_id, loop, s, rs, ok)
        self.compared["states"] += 1
        return rm, rn, rs, ok

    def score_entries(self, bow, ids):
        got = self.lib.score_entries(bow, ids)
        for k, i in enumerate(ids):
            r = self.rdb.voc.score(bow, self.w.kfs[i].mBowVec)
            assert np.float64(r).view(np.uint64) == got[k:k + 1].view(np.uint64)[0], ("library against compiled reference", i, r, got[k])
            self.compared["scores"] += 1
        return got

    def touched(self, query=0):
        return self.lib.touched(query)

    def finish(self):
        """every keyframe ever made, erased ones included: the reference's fields against the model's"""
        for k, kf in self.all:
            for loop in (False, True):
                em, en, es, _ = kf.state(loop)
                rm, rn, rs = self.rdb.fields(k, loop)
                assert (rm, rn) == (em, en) and fbits(rs) == fbits(es), (kf.mnId, loop, (rm, rn, rs), (em, en, es))
                self.compared["all_states"] += 1
        return self.compared
