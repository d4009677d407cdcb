"""The BoW transform, the six DBoW2 scores, BowVector::normalize and the keyframe database against the REFERENCE ITSELF: its
own Thirdparty/DBoW2 sources and src/KeyFrameDatabase.cc, compiled unmodified with g++ behind stand-ins for cv::Mat, KeyFrame
and Frame (oracle/ref/, libraries in oracle/_ref/; tests/ref_dbow2.py loads them).  Two builds: -O3 -ffp-contract=off stands for
fp_mode FP_STRICT, -O3 -mfma for FP_GCC_FMA.  Every comparison is exact: ids, list order, and the uint64 / uint32 bit
patterns of doubles and floats.  Compared with the compiled code are the library (host paths on a host-only handle; the device
kernels k_bow_transform, k_kfdb_common, k_kfdb_score, k_kfdb_score_slots in the GPU part), the C oracle
(oracle/orb_oracle_match.c) and the Python restatements (tests/kfdb_model.py, py_transform of tests/test_bow_transform.py).

What the first comparison showed: BowVector::normalize(L2) built with -mfma contracts `norm += v * v`; library, oracle and
restatement summed unfused under either fp_mode.  They follow fp_mode now (test_normalize_*).
One thing the reference leaves undefined: TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) passes
an uninitialised NodeId to the per-feature transform, which assigns it only when the descent passes level L - levelsup.  For a
word above that level (irregular trees) the FeatureVector entry of the reference is whatever the stack held.  The library and the
oracle file such features under node 0; the FeatureVector comparison leaves exactly those features out (and says how many).

The live tests need oracle/_ref/ (built by __graft_entry__.build() wherever the reference tree exists; it travels to machines
without one) and skip only when both are absent.  The recorded results in tests/golden/ref_dbow2_{fma,strict}.json need neither:
    python tests/test_ref_dbow2.py --record        rewrites the files from a fresh run of the compiled reference"""
import json
import os
import sys
import ctypes as C
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":      # run as a script (--record): the package and the oracle live one directory up
    sys.path.insert(0, os.path.dirname(HERE))
import oracle  # noqa: E402
import kfdb_model as M  # noqa: E402
import kfdb_driver as D  # noqa: E402
import ref_dbow2 as R  # noqa: E402
import test_kfdb as TK  # noqa: E402
import test_bow_transform as TB  # noqa: E402
from orb_slam2_detailed_comments_amd import ORBextractor, ORBVocabulary, KeyFrameDatabase, bow_score, _capi  # noqa: E402
GOLDEN = os.path.join(HERE, "golden", "ref_dbow2_%s.json")     # one file per build
MODES = [_capi.FP_GCC_FMA, _capi.FP_STRICT]
SIZES = (0, 1, 15, 16, 17, 1000)
live = pytest.mark.skipif(not R.available(), reason=R.SKIP_REASON)


def u64(x):
    return np.asarray(x, np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = u64(a), u64(b)
    return a.shape == b.shape and bool(np.all(a == b))


def mode_id(m):
    return "fma" if m == _capi.FP_GCC_FMA else "strict"


# ------------------------------------------------------------------------------------------------ scores
def score_inputs(scoring):
    """the pairs of test_kfdb.test_bow_score_all_types_bitwise, then disjoint, identical, one-word and empty vectors"""
    rng = np.random.default_rng(40 + scoring)
    out = []
    for k in range(40):
        a, b = TK.random_pair(rng, n=int(rng.integers(1, 80)))
        if k == 0:
            b = a
        if k == 1:
            b = (b[0] + np.uint32(1000), b[1])
        if scoring == M.L2_NORM:
            a = (a[0], a[1] / np.sqrt((a[1] ** 2).sum())); b = (b[0], b[1] / np.sqrt((b[1] ** 2).sum()))
        out.append((a, b))
    for k in range(6):
        a, b = TK.random_pair(rng, n=int(rng.integers(1, 80)))
        if scoring == M.L2_NORM:
            a = (a[0], a[1] / np.sqrt((a[1] ** 2).sum())); b = (b[0], b[1] / np.sqrt((b[1] ** 2).sum()))
        out.append((a, (a[0] + np.uint32(500 + k), a[1])))          # disjoint, same values: L1 gives -0.0
        out.append((a, (a[0].copy(), a[1].copy())))                 # identical: the L2 clamp
        out.append((a, (b[0][k:k + 1], b[1][k:k + 1])))             # one word against many
        out.append(((a[0][:1], a[1][:1]), (a[0][:1], a[1][:1])))    # one word against itself
    e = TK.vec([])
    out += [(e, e), (e, out[0][0]), (out[0][0], e), (TK.vec([7]), TK.vec([8])), (TK.vec([7]), TK.vec([7]))]
    return out


@live
@pytest.mark.parametrize("fp_mode", MODES, ids=mode_id)
@pytest.mark.parametrize("scoring", range(6))
def test_scores_against_compiled_reference(built_lib, scoring, fp_mode):
    ref = R.Ref(fp_mode)
    ex = TK.host_ex(fp_mode)
    neg_zero = 0
    for k, (a, b) in enumerate(score_inputs(scoring)):
        r = ref.score(scoring, a, b)
        m = M.score(scoring, a, b, fp_mode == _capi.FP_GCC_FMA)
        g = bow_score(ex, scoring, a, b)
        assert u64(r) == u64(m), ("model", scoring, k, r, m)
        assert u64(r) == u64(g), ("orbx_bow_score", scoring, k, r, g)
        neg_zero += int(u64(r) == u64(-0.0))
    if scoring == M.L1_NORM:
        assert neg_zero >= 6      # disjoint vectors: -0.0, sign bit included
    if scoring == M.L2_NORM:
        a = score_inputs(scoring)[0][0]
        assert ref.score(scoring, a, a) == 1.0


# ------------------------------------------------------------------------------------------------ normalisation
def normalize_inputs():
    """200 vectors of 1-80 words, scaled off unit norm"""
    rng = np.random.default_rng(77)
    out = []
    for _ in range(200):
        n = int(rng.integers(1, 81))
        w = np.sort(rng.choice(400, size=n, replace=False)).astype(np.uint32)
        out.append((w, (rng.random(n) + 0.01) * float(rng.uniform(0.2, 30.0))))
    return out


def tiny_vocabulary(ex, scoring, weighting=0):
    """a root with two leaves: orbx_bow_vectors needs the vocabulary's scoring, weighting and fp_mode only"""
    return ORBVocabulary(ex, n_nodes=3, k=2, L=1, child_begin=[0, 2, 2, 2], child_ids=[1, 2], desc=np.zeros((3, 32), np.uint8),
                         weight=[0.0, 1.0, 1.0], word_id=[0, 0, 1], weighting=weighting, scoring=scoring)


def lib_bow_vectors(voc, words, values):
    """orbx_bow_vectors over per-feature results (one feature per word): the BowVector values"""
    n = len(words)
    wid = np.ascontiguousarray(words, np.uint32); w = np.ascontiguousarray(values, np.float64); nid = np.zeros(max(n, 1), np.uint32)
    bw = np.zeros(max(n, 1), np.uint32); bv = np.zeros(max(n, 1), np.float64)
    fn = np.zeros(max(n, 1), np.uint32); fb = np.zeros(n + 2, np.int32); fi = np.zeros(max(n, 1), np.uint32)
    nb, nn = C.c_int(0), C.c_int(0)
    _capi.check(_capi.lib().orbx_bow_vectors(voc._h, _capi.ptr(wid), _capi.ptr(w), _capi.ptr(nid), n, _capi.ptr(bw), _capi.ptr(bv),
                                             C.byref(nb), _capi.ptr(fn), _capi.ptr(fb), _capi.ptr(fi), C.byref(nn)))
    assert np.array_equal(bw[:nb.value], wid)
    return bv[:nb.value].copy()


def oracle_bow_vectors(scoring, fp_mode, words, values):
    n = len(words)
    wid = np.ascontiguousarray(words, np.uint32); w = np.ascontiguousarray(values, np.float64); nid = np.zeros(max(n, 1), np.uint32)
    bw = np.zeros(max(n, 1), np.uint32); bv = np.zeros(max(n, 1), np.float64)
    fn = np.zeros(max(n, 1), np.uint32); fb = np.zeros(n + 2, np.int32); fi = np.zeros(max(n, 1), np.uint32)
    nb, nn = C.c_int(0), C.c_int(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    oracle.orb_oracle.lib().orc_bow_vectors(0, scoring, int(fp_mode), p(wid), p(w), p(nid), n, p(bw), p(bv), C.byref(nb), p(fn), p(fb),
                                            p(fi), C.byref(nn))
    return bv[:nb.value].copy()


@live
@pytest.mark.parametrize("fp_mode", MODES, ids=mode_id)
@pytest.mark.parametrize("norm", [1, 2], ids=["L1", "L2"])
def test_normalize_against_compiled_reference(built_lib, norm, fp_mode):
    """BowVector::normalize against orbx_bow_vectors (host-only handle), orc_bow_vectors and py_normalize"""
    ref = R.Ref(fp_mode)
    scoring = M.L1_NORM if norm == 1 else M.L2_NORM
    voc = tiny_vocabulary(TK.host_ex(fp_mode), scoring)
    bad = {"orbx_bow_vectors": [], "orc_bow_vectors": [], "py_normalize": []}
    inputs = normalize_inputs()
    for k, (w, v) in enumerate(inputs):
        r = ref.normalize((w, v), norm)
        got = {"orbx_bow_vectors": lib_bow_vectors(voc, w, v), "orc_bow_vectors": oracle_bow_vectors(scoring, fp_mode, w, v),
               "py_normalize": TB.py_normalize([float(x) for x in v], norm, fp_mode == _capi.FP_GCC_FMA)}
        for name, g in got.items():
            if not same_bits(r, g):
                bad[name].append(k)
    print("normalize %s %s: vectors differing from the compiled reference, of %d:" % ("L1 L2".split()[norm - 1], mode_id(fp_mode), len(inputs)),
          {k: len(x) for k, x in bad.items()})
    assert not any(bad.values()), bad


@live
def test_normalize_l2_is_sensitive_to_contraction():
    """non-vacuity, on the reference's outputs alone: some L2 input normalises differently in the two builds (L1 never does)"""
    fma, strict = R.Ref(_capi.FP_GCC_FMA), R.Ref(_capi.FP_STRICT)
    inputs = normalize_inputs()
    d2 = sum(not same_bits(fma.normalize(x, 2), strict.normalize(x, 2)) for x in inputs)
    d1 = sum(not same_bits(fma.normalize(x, 1), strict.normalize(x, 1)) for x in inputs)
    print("L2 inputs that normalise differently under -mfma and -ffp-contract=off: %d of %d (L1: %d)" % (d2, len(inputs), d1))
    assert d2 >= 1 and d1 == 0


# ------------------------------------------------------------------------------------------------ transform
def fv_dict(fv, drop=()):
    fn, fb, fi = fv
    out = {}
    for i in range(len(fn)):
        idx = [int(x) for x in fi[fb[i]:fb[i + 1]] if int(x) not in drop]
        if idx:
            out[int(fn[i])] = idx
    return out


def transform_feature_sets(rng, voc):
    feats = rng.integers(0, 256, (150, 32), dtype=np.uint8)
    feats[:20] = voc["desc"][rng.integers(1, voc["n_nodes"], 20)]      # the features of test_bow_transform: exact hits and ties
    sets = [feats]
    for n in SIZES:
        f = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        if n >= 16:
            f[:8] = voc["desc"][rng.integers(1, voc["n_nodes"], 8)]
        sets.append(f)
    return sets


def check_transform_against_reference(rv, got, feats, stats):
    """got and the compiled reference's transform of the same features, in the layout of oracle.bow_transform"""
    rwid, rw, rnid, (rbw, rbv), rfv = rv.transform(feats, stats["levelsup"])
    wid, w, nid, (bw, bv), fv = got
    unassigned = rnid == 0xFFFFFFFF
    assert np.array_equal(wid, rwid) and same_bits(w, rw)
    assert np.array_equal(nid, np.where(unassigned, 0, rnid).astype(np.uint32))
    assert np.array_equal(bw, rbw) and same_bits(bv, rbv)
    drop = set(int(i) for i in np.flatnonzero(unassigned))
    assert fv_dict(fv, drop) == fv_dict(rfv, drop)
    if not drop:
        assert all(np.array_equal(a, b) for a, b in zip(fv, rfv))
    stats["features"] += len(feats); stats["unassigned"] += len(drop); stats["words"] += len(bw)


@live
@pytest.mark.parametrize("k,L,irr,weighting,scoring,levelsup", TB.CASES)
def test_transform_against_compiled_reference(built_lib, tmp_path, k, L, irr, weighting, scoring, levelsup):
    rng = np.random.default_rng(k * 100 + L)
    voc, children = TB.random_vocabulary(rng, k, L, irr, weighting, scoring)
    path = str(tmp_path / "voc.txt")
    R.write_vocabulary(path, voc, children)
    sets = transform_feature_sets(rng, voc)
    # ORBVocabulary.load_text numbers nodes and words as loadFromTextFile does: its tables equal the tree that was written
    for fp_mode in MODES:
        rv = R.Ref(fp_mode).vocabulary(path)
        assert (rv.size(), rv.scoring(), rv.weighting()) == (sum(not c for c in children[1:]), scoring, weighting)
        V = ORBVocabulary.load_text(TK.host_ex(fp_mode), path)
        cb, ci, de, we, wi = V._keep
        assert np.array_equal(cb, voc["child_begin"]) and np.array_equal(ci, voc["child_ids"]) and np.array_equal(de[1:], voc["desc"][1:])
        assert same_bits(we[1:], voc["weight"][1:])
        leaf = np.array([not c for c in children])
        assert np.array_equal(wi[leaf], voc["word_id"][leaf])
        stats = dict(levelsup=levelsup, features=0, unassigned=0, words=0)
        for feats in sets:
            o = oracle.bow_transform(voc, feats, levelsup, fp_mode)
            check_transform_against_reference(rv, o, feats, stats)
            # the library's host half (orbx_bow_vectors, tables from load_text) over the per-feature results
            n = len(feats)
            bw = np.zeros(max(n, 1), np.uint32); bv = np.zeros(max(n, 1), np.float64)
            fn = np.zeros(max(n, 1), np.uint32); fb = np.zeros(n + 2, np.int32); fi = np.zeros(max(n, 1), np.uint32)
            nb, nn = C.c_int(0), C.c_int(0)
            pad = lambda a, t: np.ascontiguousarray(np.concatenate([a, np.zeros(1, t)]), t)
            _capi.check(_capi.lib().orbx_bow_vectors(V._h, _capi.ptr(pad(o[0], np.uint32)), _capi.ptr(pad(o[1], np.float64)),
                                                     _capi.ptr(pad(o[2], np.uint32)), n, _capi.ptr(bw), _capi.ptr(bv), C.byref(nb),
                                                     _capi.ptr(fn), _capi.ptr(fb), _capi.ptr(fi), C.byref(nn)))
            g = (o[0], o[1], o[2], (bw[:nb.value], bv[:nb.value]), (fn[:nn.value], fb[:nn.value + 1], fi[:fb[nn.value]]))
            check_transform_against_reference(rv, g, feats, stats)
            if len(feats) <= 150:   # the Python restatement is slow
                per, (keys, vals), pfv = TB.py_transform(voc, children, feats, levelsup, fp_mode == _capi.FP_GCC_FMA)
                p = (np.array([x[0] for x in per], np.uint32), np.array([x[1] for x in per], np.float64),
                     np.array([x[2] for x in per], np.uint32), (np.array(keys, np.uint32), np.array(vals, np.float64)),
                     (np.array(list(pfv), np.uint32), np.cumsum([0] + [len(x) for x in pfv.values()]).astype(np.int32),
                      np.array([i for x in pfv.values() for i in x], np.uint32)))
                check_transform_against_reference(rv, p, feats, stats)
        print("transform", (k, L, irr, weighting, scoring, levelsup), mode_id(fp_mode), stats)
        assert stats["words"] > 0 and (irr or stats["unassigned"] == 0)


# ------------------------------------------------------------------------------------------------ keyframe database
class RefMake:
    """stands in for test_kfdb.make: the same Checked, its database a Tee over the library database and the compiled one"""

    def __init__(self, fp_mode=None):
        self.fp_mode, self.tees = fp_mode, []

    def __call__(self, ex, seed=0, scoring=M.L1_NORM, fma_mode=True, **kw):
        fp_mode = ex.params.fp_mode
        assert (fp_mode == _capi.FP_GCC_FMA) == fma_mode
        w = D.World(seed, scoring=scoring, fma_mode=fma_mode, **kw)
        tee = R.Tee(w, KeyFrameDatabase(ex, scoring=scoring), R.Ref(fp_mode))
        self.tees.append(tee)
        return D.Checked(w, tee)

    def finish(self):
        total = {}
        for t in self.tees:
            for k, v in t.finish().items():
                total[k] = total.get(k, 0) + v
        assert total["candidates"] > 0 and total["states"] > 0 and total["all_states"] > 0, total
        return total


@pytest.fixture
def ref_make(monkeypatch):
    mk = RefMake()
    monkeypatch.setattr(TK, "make", mk)    # the hand-worked cases of test_kfdb.py call make(ex) themselves
    return mk


@live
@pytest.mark.parametrize("case", TK.HAND_CASES, ids=lambda f: f.__name__)
def test_kfdb_hand_cases_against_compiled_reference(built_lib, ref_make, case):
    case(TK.host_ex())
    print(case.__name__, ref_make.finish())


@live
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_kfdb_seeded_sequences_against_compiled_reference(built_lib, ref_make, seed):
    c = ref_make(TK.host_ex(), seed)
    st = D.play(c, 70, 100 + seed)
    D.assert_not_vacuous(st)
    total = ref_make.finish()
    print("seed", seed, st, total)
    assert total["scores"] > 0


@live
@pytest.mark.parametrize("scoring", [M.L2_NORM, M.CHI_SQUARE, M.KL, M.BHATTACHARYYA, M.DOT_PRODUCT])
def test_kfdb_other_scoring_types_against_compiled_reference(built_lib, ref_make, scoring):
    for fp_mode in MODES:
        c = ref_make(TK.host_ex(fp_mode), 10 + scoring, scoring=scoring, fma_mode=fp_mode == _capi.FP_GCC_FMA)
        D.play(c, 25, 200 + scoring)
    print("scoring", scoring, ref_make.finish())


# ------------------------------------------------------------------------------------------------ recorded results
GOLDEN_SEQ = dict(seed=6, steps=14, play_seed=66)


class Recorder(R.Tee):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.log = []

    def select_groups(self, query, neighbours):
        out = super().select_groups(query, neighbours)
        self.log.append([int(i) for i in out[0]])
        return out

    def final(self):
        return [[int(kf.mnId)] + [int(x) for loop in (False, True) for x in
                                  (lambda m, n, s: (m, n, int(R.fbits(s))))(*self.rdb.fields(k, loop))] for k, kf in self.all]


class Replay:
    """the `db` of a Checked without the compiled reference: the library's candidates against the recorded ones, call by call"""

    def __init__(self, world, lib, rec):
        self.w, self.lib, self.rec, self.pos, self.all = world, lib, rec, 0, []

    def __getattr__(self, name):
        return getattr(self.lib, name)

    def __len__(self):
        return len(self.lib)

    def add(self, kf_id, bow):
        self.lib.add(kf_id, bow)
        self.all.append(self.w.kfs[kf_id])

    def select_groups(self, query, neighbours):
        cand, unscored = self.lib.select_groups(query, neighbours)
        assert [int(i) for i in cand] == self.rec["candidates"][self.pos], (self.pos, list(cand), self.rec["candidates"][self.pos])
        self.pos += 1
        return cand, unscored

    def finish(self):
        assert self.pos == len(self.rec["candidates"]) and len(self.all) == len(self.rec["final"])
        for kf, row in zip(self.all, self.rec["final"]):
            got = [kf.mnId] + [int(x) for loop in (False, True) for x in (lambda m, n, s, ok: (m, n, int(R.fbits(s))))(*kf.state(loop))]
            assert got == row, (got, row)             # the model's keyframes, erased ones included
            if kf.mnId in self.w.kfs and self.w.kfs[kf.mnId] is kf:
                for f, loop in enumerate((False, True)):
                    m, n, s, ok = self.lib.state(kf.mnId, loop)
                    assert [m, n, int(R.fbits(s)) if ok else 0] == row[1 + 3 * f: 4 + 3 * f], (kf.mnId, loop)


def golden_score_inputs():
    return [(s, k, a, b) for s in range(6) for k, (a, b) in enumerate(score_inputs(s)) if k < 4 or k >= 40][:300]


def hexbits(x):
    return ["%016x" % int(v) for v in u64(x).reshape(-1)]


def record():
    """everything the golden file holds, from a fresh run of the compiled reference"""
    info = open(os.path.join(R.build_ref.OUT, "BUILD_INFO.txt")).read().splitlines()
    out = {}
    for fp_mode in MODES:
        ref = R.Ref(fp_mode)
        rec = {"scores": [hexbits(ref.score(s, a, b))[0] for s, k, a, b in golden_score_inputs()],
               "normalize_l1": [hexbits(ref.normalize(x, 1)) for x in normalize_inputs()[:12]],
               "normalize_l2": [hexbits(ref.normalize(x, 2)) for x in normalize_inputs()[:12]]}
        ex = TK.host_ex(fp_mode)
        w = D.World(GOLDEN_SEQ["seed"], fma_mode=fp_mode == _capi.FP_GCC_FMA)
        tee = Recorder(w, KeyFrameDatabase(ex, scoring=M.L1_NORM), ref)
        D.play(D.Checked(w, tee), GOLDEN_SEQ["steps"], GOLDEN_SEQ["play_seed"])
        tee.finish()
        rec["candidates"], rec["final"] = tee.log, tee.final()
        rec["generator"] = "python tests/test_ref_dbow2.py --record"
        rec["build"] = [info[0]] + [x for x in info if x.startswith("libref_dbow2_%s" % mode_id(fp_mode))]
        out[mode_id(fp_mode)] = rec
    return out


@pytest.fixture(scope="module")
def golden():
    out = {}
    for m in ("fma", "strict"):
        with open(GOLDEN % m) as f:
            out[m] = json.load(f)
    return out


@pytest.mark.parametrize("fp_mode", MODES, ids=mode_id)
def test_recorded_scores_and_normalisation(built_lib, golden, fp_mode):
    """needs no compiled reference: library, oracle and restatements against what the compiled reference gave when recorded"""
    rec = golden[mode_id(fp_mode)]
    ex = TK.host_ex(fp_mode)
    fma_mode = fp_mode == _capi.FP_GCC_FMA
    inputs = golden_score_inputs()
    assert len(inputs) == len(rec["scores"]) >= 36
    for (s, k, a, b), bits in zip(inputs, rec["scores"]):
        assert hexbits(bow_score(ex, s, a, b))[0] == bits, (s, k)
        assert hexbits(M.score(s, a, b, fma_mode))[0] == bits, (s, k)
    for norm, key in ((1, "normalize_l1"), (2, "normalize_l2")):
        scoring = M.L1_NORM if norm == 1 else M.L2_NORM
        voc = tiny_vocabulary(ex, scoring)
        for (w, v), bits in zip(normalize_inputs(), rec[key]):
            assert hexbits(lib_bow_vectors(voc, w, v)) == bits
            assert hexbits(oracle_bow_vectors(scoring, fp_mode, w, v)) == bits
            assert hexbits(TB.py_normalize([float(x) for x in v], norm, fma_mode)) == bits


def test_recorded_normalisation_tells_the_builds_apart(golden):
    assert golden["fma"]["normalize_l2"] != golden["strict"]["normalize_l2"]
    assert golden["fma"]["normalize_l1"] == golden["strict"]["normalize_l1"]


@pytest.mark.parametrize("fp_mode", MODES, ids=mode_id)
def test_recorded_sequence(built_lib, golden, fp_mode):
    rec = golden[mode_id(fp_mode)]
    w = D.World(GOLDEN_SEQ["seed"], fma_mode=fp_mode == _capi.FP_GCC_FMA)
    rp = Replay(w, KeyFrameDatabase(TK.host_ex(fp_mode), scoring=M.L1_NORM), rec)
    D.play(D.Checked(w, rp), GOLDEN_SEQ["steps"], GOLDEN_SEQ["play_seed"])
    rp.finish()
    assert any(rec["candidates"]) and len(rec["final"]) > 70


@live
def test_compiled_reference_reproduces_the_recorded_file(built_lib, golden):
    fresh = record()
    for m in ("fma", "strict"):
        for key in ("scores", "normalize_l1", "normalize_l2", "candidates", "final"):
            assert fresh[m][key] == golden[m][key], (m, key)


# ------------------------------------------------------------------------------------------------ GPU part
# These load oracle/_ref/*.so and files under tests/ only.
@pytest.fixture(scope="module")
def dev_exs():
    return {m: ORBextractor(1000, 1.2, 8, 20, 7, device=0, fp_mode=m) for m in MODES}


@live
@pytest.mark.gpu
@pytest.mark.parametrize("k,L,irr,weighting,scoring,levelsup", TB.CASES)
def test_gpu_transform_against_compiled_reference(dev_exs, tmp_path, k, L, irr, weighting, scoring, levelsup):
    """k_bow_transform + orbx_bow_vectors against the compiled transform"""
    rng = np.random.default_rng(k * 100 + L)
    voc, children = TB.random_vocabulary(rng, k, L, irr, weighting, scoring)
    path = str(tmp_path / "voc.txt")
    R.write_vocabulary(path, voc, children)
    sets = transform_feature_sets(rng, voc)
    for fp_mode in MODES:
        rv = R.Ref(fp_mode).vocabulary(path)
        stats = dict(levelsup=levelsup, features=0, unassigned=0, words=0)
        for V in (ORBVocabulary(dev_exs[fp_mode], **voc), ORBVocabulary.load_text(dev_exs[fp_mode], path)):
            for feats in sets:
                wid, w, nid = V.transform_features(feats, levelsup)
                bowv, fv = V.transform(feats, levelsup)
                check_transform_against_reference(rv, (wid, w, nid, bowv, fv), feats, stats)
        assert stats["words"] > 0


@pytest.fixture
def gpu_ref_make(monkeypatch):
    mk = RefMake()
    monkeypatch.setattr(TK, "make", mk)
    return mk


@live
@pytest.mark.gpu
@pytest.mark.parametrize("case", TK.HAND_CASES, ids=lambda f: f.__name__)
def test_gpu_kfdb_hand_cases_against_compiled_reference(dev_exs, gpu_ref_make, case):
    case(dev_exs[_capi.FP_GCC_FMA])
    gpu_ref_make.finish()


@live
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_gpu_kfdb_seeded_sequences_against_compiled_reference(dev_exs, gpu_ref_make, seed):
    c = gpu_ref_make(dev_exs[_capi.FP_GCC_FMA], seed)
    D.assert_not_vacuous(D.play(c, 70, 100 + seed))
    assert gpu_ref_make.finish()["scores"] > 0


@live
@pytest.mark.gpu
@pytest.mark.parametrize("fp_mode", MODES, ids=mode_id)
@pytest.mark.parametrize("scoring", TK.DEVICE_TYPES)
def test_gpu_kfdb_scoring_types_against_compiled_reference(dev_exs, gpu_ref_make, scoring, fp_mode):
    """whole sequences per device scoring type and fp_mode, then score_entries (k_kfdb_score_slots) against the compiled score
    for 300 entries"""
    ex, ref = dev_exs[fp_mode], R.Ref(fp_mode)
    c = gpu_ref_make(ex, 20 + scoring, scoring=scoring, fma_mode=fp_mode == _capi.FP_GCC_FMA)
    D.play(c, 25, 300 + scoring)
    gpu_ref_make.finish()
    rng = np.random.default_rng(70 + scoring)
    db = KeyFrameDatabase(ex, scoring=scoring)
    vs = []
    for i in range(300):
        a, _ = TK.random_pair(rng, n=int(rng.integers(1, 200)), vocab=400)
        if scoring == M.L2_NORM:
            a = (a[0], a[1] / np.sqrt((a[1] ** 2).sum()))
        vs.append(a); db.add(i, a)
    for q in (vs[0], vs[7], TK.random_pair(rng, n=150, vocab=400)[0]):
        got = db.score_entries(q, np.arange(300))
        exp = np.array([ref.score(scoring, q, v) for v in vs])
        assert same_bits(got, exp), (scoring, np.flatnonzero(u64(got) != u64(exp))[:5])


@live
@pytest.mark.gpu
def test_gpu_kfdb_batched_call_against_sequential_reference_calls(dev_exs, gpu_ref_make):
    """24 relocalisation queries in ONE library call; the compiled reference runs them one after the other"""
    a = gpu_ref_make(dev_exs[_capi.FP_GCC_FMA], 9)
    D.build_map(a)
    places = [int(x) for x in np.random.default_rng(4).integers(0, a.w.places, size=24)]
    rs = a.reloc(places)
    assert len(a.db.cands) == 24 and all(r.candidates for r in rs)
    st = a.w.stats
    assert st["stale"] >= 1 and st["unscored"] >= 1, st
    assert gpu_ref_make.finish()["candidates"] == 24


@live
@pytest.mark.gpu
def test_gpu_kfdb_long_vectors_against_compiled_reference(dev_exs, gpu_ref_make):
    """the long-vector case of test_kfdb.test_extremes: vectors past the 4096-word LDS staging of the query"""
    rng = np.random.default_rng(12)
    c = gpu_ref_make(dev_exs[_capi.FP_GCC_FMA], 12, places=4, words=48, vocab=40000)
    D.build_map(c)

    def long_vec(n):
        w = np.sort(rng.choice(40000, size=n, replace=False)).astype(np.uint32)
        v = rng.random(n) + 0.01
        return w, v / v.sum()
    big = [long_vec(5000), long_vec(9000)]
    c.add(1, bow=big[0]); c.add(2, bow=big[1])
    rs = c.reloc([long_vec(6000), big[1], (big[0][0][:4096], big[0][1][:4096]), (big[0][0][:4097], big[0][1][:4097])])
    assert all(r.sharing for r in rs) and rs[1].score_and_match
    c.loop(1, bow=long_vec(4500), same_place=True)
    gpu_ref_make.finish()


@live
@pytest.mark.gpu
def test_gpu_chain_from_descriptors_against_compiled_reference(dev_exs, tmp_path):
    """extract -> transform on the device next to the compiled transform -> add -> query on both sides"""
    from orb_slam2_detailed_comments_amd import synth
    ex, ref = dev_exs[_capi.FP_GCC_FMA], R.Ref(_capi.FP_GCC_FMA)
    rng = np.random.default_rng(15)
    frames = synth.stream(640, 480, 6, stream_id=52)
    ex6 = ORBextractor(1000, max_batch=6)
    descs = [d for _, d in ex6.extract_batch(frames)]
    voc, children = TB.random_vocabulary(rng, 8, 3, False, scoring=M.L1_NORM, stop=0.0)
    voc["desc"][1:] = descs[0][rng.integers(0, len(descs[0]), voc["n_nodes"] - 1)]
    path = str(tmp_path / "voc.txt")
    R.write_vocabulary(path, voc, children)
    V, rv = ORBVocabulary.load_text(ex, path), ref.vocabulary(path)
    w = D.World(15)                                  # book-keeping only: every vector below comes from the transform
    tee = R.Tee(w, KeyFrameDatabase(ex, V), ref, voc=rv)
    c = D.Checked(w, tee); w.covis = {}
    stats = dict(levelsup=4, features=0, unassigned=0, words=0)

    def bow(d):
        wid, wt, nid = V.transform_features(d, 4)
        bowv, fv = V.transform(d, 4)
        check_transform_against_reference(rv, (wid, wt, nid, bowv, fv), d, stats)
        return bowv
    for i, d in enumerate(descs[:5]):
        c.add(0, kf_id=i + 1, bow=bow(d))
    w.covis = {i: [j for j in range(1, 6) if abs(j - i) == 1] for i in range(1, 6)}
    r, = c.reloc([bow(descs[5])], frame_ids=[40])
    assert r.candidates and stats["unassigned"] == 0
    c.loop(0, kf_id=41, bow=bow(descs[2][::2]), connected=[3], min_score=0.0, add_after=False)
    assert tee.finish()["candidates"] == 2


if __name__ == "__main__":
    if "--record" in sys.argv:
        assert R.available(), R.SKIP_REASON
        for m, rec in record().items():
            with open(GOLDEN % m, "w") as f:
                json.dump(rec, f, separators=(",", ":"))
                f.write("\n")
            print("wrote", GOLDEN % m, os.path.getsize(GOLDEN % m), "bytes")
