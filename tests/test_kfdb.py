"""Keyframe database (include/orbx.h: orbx_kfdb_*, orbx_bow_score) against tests/kfdb_model.py, the restatement of the
reference's src/KeyFrameDatabase.cc:56-411 and Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-315.

Every comparison is exact: candidate ids and order, lScoreAndMatch ids and order, score bit patterns, minCommonWords, the count
of reads of never-written scores and the per-entry marks / word counts / scores after every call.
The model itself, the host path and the device path are pinned to the compiled reference by tests/test_ref_dbow2.py, which
replays HAND_CASES and the seeded sequences of this file on the reference's own KeyFrameDatabase.  CPU part: the model against hand-worked cases, and the
library's host path (host-only handle) against the model.  GPU part: the device path (k_kfdb_common / k_kfdb_score), the
host path on a device handle, batched against single calls, every device scoring type, the extremes, and one chain from
descriptors.  The sequences come from tests/kfdb_driver.py, which asserts on the MODEL's output that they exercise stale
and never-scored reads, minScore rejections and connected keyframes before anything is compared."""
import os
import subprocess
import numpy as np
import pytest
import kfdb_model as M
import kfdb_driver as D
from orb_slam2_detailed_comments_amd import ORBextractor, KeyFrameDatabase, OrbxError, bow_score, _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEVICE_TYPES = (M.L1_NORM, M.L2_NORM, M.CHI_SQUARE, M.BHATTACHARYYA, M.DOT_PRODUCT)


def host_ex(fp_mode=_capi.FP_GCC_FMA):
    return ORBextractor(1000, 1.2, 8, 20, 7, device=-2, fp_mode=fp_mode)


def make(ex, seed=0, scoring=M.L1_NORM, fma_mode=True, **kw):
    w = D.World(seed, scoring=scoring, fma_mode=fma_mode, **kw)
    return D.Checked(w, KeyFrameDatabase(ex, scoring=scoring))


def vec(words, values=None):
    w = np.asarray(words, np.uint32)
    v = np.full(len(w), 1.0 / max(len(w), 1)) if values is None else np.asarray(values, np.float64)
    return w, v


def u64(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ hand-worked cases
# Each runs on the model AND (through D.Checked, which compares the two) on a library database of the given extractor, so the
# GPU part reuses them on the device path.
def case_list_order(ex):
    """lKFsSharingWords = first encounter: ascending query word, each word's list in add order; erase keeps the others' order"""
    c = make(ex); c.w.covis = {}
    c.add(0, kf_id=1, bow=vec([5, 9])); c.add(0, kf_id=2, bow=vec([3, 9])); c.add(0, kf_id=3, bow=vec([5, 9]))
    r, = c.reloc([vec([3, 5, 9])], frame_ids=[100])
    assert [k.mnId for k in r.sharing] == [2, 1, 3] and [k.mnId for _, k in r.score_and_match] == [2, 1, 3]
    c.erase(1); c.add(0, kf_id=4, bow=vec([5, 9]))          # word 5: [3, 4], word 9: [2, 3, 4]
    r, = c.reloc([vec([3, 5, 9])], frame_ids=[101])
    assert [k.mnId for k in r.sharing] == [2, 3, 4]
    c.add(0, kf_id=1, bow=vec([4, 5]))                       # the erased id comes back as a new keyframe, last in every list
    r, = c.reloc([vec([4, 5, 9])], frame_ids=[102])
    assert [k.mnId for k in r.sharing] == [1, 3, 4, 2]
    assert c.db.state(1)[:2] == (102, 2)


def case_connected_ends_at_one_word(ex):
    c = make(ex); c.w.covis = {}
    c.add(0, kf_id=1, bow=vec([1, 2, 3, 4])); c.add(0, kf_id=2, bow=vec([1, 2, 3, 9]))
    r = c.loop(0, kf_id=50, bow=vec([1, 2, 3, 4]), connected=[1], min_score=0.0, add_after=False)
    assert [k.mnId for k in r.sharing] == [2] and r.connected_met == 4   # met once per common word
    assert c.db.state(1, True)[:2] == (0, 1)                 # never marked, reset and incremented at every encounter
    assert c.db.state(2, True)[:2] == (50, 3)


def case_id_zero_and_repeated_id(ex):
    c = make(ex); c.w.covis = {}
    c.add(0, kf_id=1, bow=vec([1, 2, 3])); c.add(0, kf_id=2, bow=vec([2, 3, 4]))
    r, = c.reloc([vec([1, 2, 3])], frame_ids=[0])            # fresh marks are 0 == the query id: nothing is listed
    assert not r.sharing and not r.candidates
    assert c.db.state(1)[:2] == (0, 3) and c.db.state(2)[:2] == (0, 2)
    r, = c.reloc([vec([1, 2, 3])], frame_ids=[7])
    assert [k.mnId for k in r.sharing] == [1, 2] and c.db.state(1)[:2] == (7, 3)
    r, = c.reloc([vec([1, 2, 3])], frame_ids=[7])            # the same id again: not re-listed, the counts continue
    assert not r.sharing and not r.candidates
    assert c.db.state(1)[:2] == (7, 6) and c.db.state(2)[:2] == (7, 4)
    r = c.reloc([vec([2, 3]), vec([2, 3])], frame_ids=[8, 8])   # ... and inside one batched call
    assert [k.mnId for k in r[0].sharing] == [1, 2] and not r[1].sharing
    assert c.db.state(1)[:2] == (8, 4)
    # loop form: an entry already marked with the query id keeps counting even when it is connected now
    c.loop(0, kf_id=60, bow=vec([1, 2, 3]), connected=[], min_score=0.0, add_after=False)
    r = c.loop(0, kf_id=60, bow=vec([1, 2, 3]), connected=[1], min_score=0.0, add_after=False)
    assert not r.sharing and c.db.state(1, True)[:2] == (60, 6)


def case_stale_and_unscored_reads(ex):
    """F8: step 4 of the relocalisation form adds mRelocScore of every neighbour the query marked, scored or not"""
    X, N = vec([1, 2, 3, 4, 5]), vec([5, 10, 11, 12, 13])
    q2 = vec([1, 2, 3, 4, 5], [.1, .3, .2, .2, .2])

    def fresh():
        c = make(ex); c.w.covis = {1: [2], 2: [1]}
        c.add(0, kf_id=1, bow=X); c.add(0, kf_id=2, bow=N)
        return c
    c = fresh()
    r, = c.reloc([q2], frame_ids=[12])                        # N shares one word: marked, below the threshold, never scored
    assert [k.mnId for k in r.candidates] == [1] and (r.unscored_reads, r.stale_reads) == (1, 0)
    assert c.db.state(2) == (12, 1, np.float32(0), 0)
    c = fresh()
    r, = c.reloc([N], frame_ids=[11])                         # first a query that scores N (identical vector: 1.0)
    assert [k.mnId for k in r.candidates] == [2] and r.unscored_reads == 1
    assert c.db.state(2)[2:] == (np.float32(1), 1)
    r, = c.reloc([q2], frame_ids=[12])                        # the stale 1.0 of N beats X's own 0.9: the winner changes
    assert [k.mnId for _, k in r.score_and_match] == [1]
    assert [k.mnId for k in r.candidates] == [2] and (r.unscored_reads, r.stale_reads) == (0, 1)
    # the same two queries in ONE call: the groups of query 0 must not see the state query 1 leaves
    c = fresh()
    r = c.reloc([N, q2], frame_ids=[11, 12])
    assert [k.mnId for k in r[0].candidates] == [2] and r[0].unscored_reads == 1
    assert [k.mnId for k in r[1].candidates] == [2] and r[1].stale_reads == 1


def case_min_score_equality(ex):
    c = make(ex); c.w.covis = {}
    a, q = vec([1, 2, 3, 4], [.1, .2, .3, .4]), vec([1, 2, 3, 4], [.4, .3, .2, .1])
    c.add(0, kf_id=1, bow=a)
    si = np.float32(M.score(M.L1_NORM, q, a))
    r = c.loop(0, kf_id=70, bow=q, connected=[], min_score=si, add_after=False)
    assert [k.mnId for _, k in r.score_and_match] == [1] and r.rejected_min_score == 0      # si >= minScore holds at equality
    r = c.loop(0, kf_id=71, bow=q, connected=[], min_score=np.nextafter(si, np.float32(2)), add_after=False)
    assert not r.score_and_match and r.rejected_min_score == 1 and not r.candidates
    assert c.db.state(1, True) == (71, 4, si, 1)             # scored and stored all the same


def case_dedup_first_occurrence(ex):
    c = make(ex); c.w.covis = {1: [2], 2: [1, 3], 3: [2]}
    q = vec([1, 2, 3, 4, 5, 6])
    c.add(0, kf_id=1, bow=vec([1, 2, 3, 4, 5, 7])); c.add(0, kf_id=2, bow=q); c.add(0, kf_id=3, bow=vec([2, 3, 4, 5, 6, 8]))
    r, = c.reloc([q], frame_ids=[9])
    assert [k.mnId for _, k in r.score_and_match] == [1, 2, 3]
    assert [k.mnId for k in r.candidates] == [2]             # best member of all three groups, kept once


HAND_CASES = [case_list_order, case_connected_ends_at_one_word, case_id_zero_and_repeated_id, case_stale_and_unscored_reads,
              case_min_score_equality, case_dedup_first_occurrence]


# ------------------------------------------------------------------------------------------------ CPU part
@pytest.mark.parametrize("case", HAND_CASES, ids=lambda f: f.__name__)
def test_hand_worked_cases_host_path(built_lib, case):
    case(host_ex())


def test_min_common_words_truncation_identity():
    """`int minCommonWords = maxCommonWords * 0.8f`: no word count a vector can reach tells the float form from the integer or
    the double form; the library keeps the reference's float form"""
    m = np.arange(200000)
    f = (m.astype(np.float32) * np.float32(0.8)).astype(np.int64)
    assert np.array_equal(f, (4 * m) // 5) and np.array_equal(f, (m * 0.8).astype(np.int64))
    assert all(M.min_common_words(int(x)) == int(f[x]) for x in (0, 1, 4, 5, 6, 1999, 199999))


def random_pair(rng, n=60, vocab=150):
    out = []
    for _ in range(2):
        w = np.unique(rng.integers(0, vocab, size=n).astype(np.uint32))
        v = rng.random(len(w)) + 1e-3
        out.append((w, v / v.sum()))
    return out


@pytest.mark.parametrize("fp_mode", [_capi.FP_GCC_FMA, _capi.FP_STRICT])
@pytest.mark.parametrize("scoring", range(6))
def test_bow_score_all_types_bitwise(built_lib, scoring, fp_mode):
    ex = host_ex(fp_mode)
    rng = np.random.default_rng(40 + scoring)
    for k in range(40):
        a, b = random_pair(rng, n=int(rng.integers(1, 80)))
        if k == 0:
            b = a                                             # identical vectors: the L2 clamp, sqrt of squares
        if k == 1:
            b = (b[0] + np.uint32(1000), b[1])                # no common word
        if scoring == M.L2_NORM:                              # L2-normalised, as DBoW2 keeps them for this type
            a = (a[0], a[1] / np.sqrt((a[1] ** 2).sum())); b = (b[0], b[1] / np.sqrt((b[1] ** 2).sum()))
        got = bow_score(ex, scoring, a, b)
        exp = M.score(scoring, a, b, fp_mode == _capi.FP_GCC_FMA)
        assert u64(got) == u64(exp), (scoring, k, got, exp)
    assert bow_score(ex, scoring, vec([]), vec([1])) == M.score(scoring, vec([]), vec([1]))


def test_fma_mode_is_observable_in_the_product_types():
    """the fused and the unfused sums differ for some input (otherwise fp_mode would be untestable); L1 has no product"""
    rng = np.random.default_rng(3)
    diff = {s: 0 for s in (M.L1_NORM, M.L2_NORM, M.DOT_PRODUCT)}
    for _ in range(50):
        a, _ = random_pair(rng)
        b = (a[0], a[1] * (1 + 0.1 * rng.random(len(a[1]))))   # near-identical, L2-normalised: 1 - score keeps the last bits
        a = (a[0], a[1] / np.sqrt((a[1] ** 2).sum())); b = (b[0], b[1] / np.sqrt((b[1] ** 2).sum()))
        for s in diff:
            diff[s] += M.score(s, a, b, True) != M.score(s, a, b, False)
    assert diff[M.L1_NORM] == 0 and diff[M.L2_NORM] > 0 and diff[M.DOT_PRODUCT] > 0


def test_argument_validation_host_only(built_lib):
    ex = host_ex()
    with pytest.raises(OrbxError) as e:
        KeyFrameDatabase(ex, scoring=6)
    assert e.value.status == _capi.BAD_ARGUMENT
    db = KeyFrameDatabase(ex, scoring=M.L1_NORM)
    db.add(1, vec([1, 2, 3]))
    for bad in (lambda: db.add(1, vec([4])),                  # duplicate id
                lambda: db.erase(2),                          # unknown id
                lambda: db.add(3, vec([2, 2])),               # words must ascend strictly
                lambda: db.add(3, vec([3, 2])),
                lambda: db.state(9),
                lambda: db.score_entries(vec([1]), [9]),
                lambda: db.query_reloc([5], [vec([2, 1])]),
                lambda: db.select_groups(0, [])):             # no query yet
        with pytest.raises(OrbxError) as e:
            bad()
        assert e.value.status == _capi.BAD_ARGUMENT
    assert len(db) == 1
    got = db.query_reloc([5, 6], [vec([1, 2]), vec([3])])
    assert [list(g[0]) for g in got] == [[1], [1]]
    with pytest.raises(OrbxError):
        db.select_groups(1, [[]])                             # out of order
    assert list(db.select_groups(0, [[]])[0]) == [1]
    with pytest.raises(OrbxError):
        db.select_groups(0, [[]])                             # once per query
    assert list(db.touched(1)) == [1]
    db.state(1)                                               # any other call ends the batch ...
    with pytest.raises(OrbxError):
        db.select_groups(1, [[]])
    assert db.state(1)[:2] == (6, 1)                          # ... and query 1 still left its state
    db.clear()
    assert len(db) == 0 and db.query_reloc([7], [vec([1])])[0][0].size == 0
    db.add(1, vec([]))                                        # an empty BowVector is an entry no query meets
    assert db.query_reloc([8], [vec([1])])[0][0].size == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_path_seeded_sequences(built_lib, seed):
    c = make(host_ex(), seed)
    st = D.play(c, 70, 100 + seed)
    D.assert_not_vacuous(st)


@pytest.mark.parametrize("scoring", [M.L2_NORM, M.CHI_SQUARE, M.KL, M.BHATTACHARYYA, M.DOT_PRODUCT])
def test_host_path_other_scoring_types(built_lib, scoring):
    for fp_mode in (_capi.FP_GCC_FMA, _capi.FP_STRICT):
        c = make(host_ex(fp_mode), 10 + scoring, scoring=scoring, fma_mode=fp_mode == _capi.FP_GCC_FMA)
        D.play(c, 25, 200 + scoring)


# ------------------------------------------------------------------------------------------------ GPU part
@pytest.fixture(scope="module")
def dev_ex():
    return ORBextractor(1000, 1.2, 8, 20, 7, device=0)


@pytest.fixture
def host_switch(monkeypatch):
    monkeypatch.setenv("ORBX_KFDB", "host")


@pytest.mark.gpu
@pytest.mark.parametrize("case", HAND_CASES, ids=lambda f: f.__name__)
def test_hand_worked_cases_device(dev_ex, case):
    case(dev_ex)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HAND_CASES, ids=lambda f: f.__name__)
def test_hand_worked_cases_host_switch_on_device_handle(dev_ex, host_switch, case):
    case(dev_ex)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_device_seeded_sequences(dev_ex, seed):
    c = make(dev_ex, seed)
    st = D.play(c, 70, 100 + seed)
    D.assert_not_vacuous(st)


@pytest.mark.gpu
def test_device_path_against_host_path(dev_ex, monkeypatch):
    """the same sequence on two databases of one device handle, one of them behind ORBX_KFDB=host: both equal the model"""
    for path in ("device", "host"):
        monkeypatch.setenv("ORBX_KFDB", path)
        c = make(dev_ex, 5)
        D.assert_not_vacuous(D.play(c, 50, 55))


@pytest.mark.gpu
@pytest.mark.parametrize("fp_mode", [_capi.FP_GCC_FMA, _capi.FP_STRICT])
@pytest.mark.parametrize("scoring", DEVICE_TYPES)
def test_device_scoring_types(scoring, fp_mode):
    """every device scoring type against orbx_bow_score (bitwise, double) and through whole queries against the model"""
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=0, fp_mode=fp_mode)
    fma_mode = fp_mode == _capi.FP_GCC_FMA
    rng = np.random.default_rng(70 + scoring)
    db = KeyFrameDatabase(ex, scoring=scoring)
    vs = []
    for i in range(300):
        a, _ = random_pair(rng, n=int(rng.integers(1, 200)), vocab=400)
        if scoring == M.L2_NORM:
            a = (a[0], a[1] / np.sqrt((a[1] ** 2).sum()))
        vs.append(a); db.add(i, a)
    for q in (vs[0], vs[7], random_pair(rng, n=150, vocab=400)[0]):
        got = db.score_entries(q, np.arange(300))
        exp = np.array([bow_score(ex, scoring, q, v) for v in vs])
        assert np.array_equal(u64(got), u64(exp)), (scoring, np.flatnonzero(u64(got) != u64(exp))[:5])
        assert u64(exp[0]) == u64(M.score(scoring, q, vs[0], fma_mode))
    c = make(ex, 20 + scoring, scoring=scoring, fma_mode=fma_mode)
    D.play(c, 25, 300 + scoring)


@pytest.mark.gpu
def test_kl_is_host_only(dev_ex, monkeypatch):
    db = KeyFrameDatabase(dev_ex, scoring=M.KL)
    db.add(1, vec([1, 2]))
    with pytest.raises(OrbxError) as e:
        db.query_reloc([1], [vec([1])])
    assert e.value.status == _capi.UNSUPPORTED
    with pytest.raises(OrbxError) as e:
        db.score_entries(vec([1]), [1])
    assert e.value.status == _capi.UNSUPPORTED
    monkeypatch.setenv("ORBX_KFDB", "host")
    assert u64(db.score_entries(vec([1]), [1])[0]) == u64(M.score(M.KL, vec([1]), vec([1, 2])))


@pytest.mark.gpu
def test_batched_call_equals_single_calls(dev_ex):
    """nqueries = Q in one call against Q single calls: two databases, both against the model, then against each other"""
    Q = 24
    a, b = make(dev_ex, 9), make(dev_ex, 9)
    D.build_map(a); D.build_map(b)
    places = [int(x) for x in np.random.default_rng(4).integers(0, a.w.places, size=Q)]
    ra = a.reloc(places)                                      # one call (same seed: the same vectors in both worlds)
    rb = [b.reloc([p])[0] for p in places]
    D.assert_not_vacuous({**a.w.stats, "loop": 1, "rejected_min_score": 1, "connected_met": 1})
    for x, y in zip(ra, rb):
        assert [k.mnId for k in x.candidates] == [k.mnId for k in y.candidates]
        assert [k.mnId for _, k in x.score_and_match] == [k.mnId for _, k in y.score_and_match]
    for i in a.w.kfs:
        assert a.db.state(i) == b.db.state(i)


@pytest.mark.gpu
def test_extremes(dev_ex):
    c = make(dev_ex, 11); c.w.covis = {}
    r, = c.reloc([vec([1, 2, 3])], frame_ids=[1])             # an empty database
    assert not r.sharing
    assert c.db.score_entries(vec([1]), []).size == 0
    c.add(0, kf_id=1, bow=vec([7])); c.add(0, kf_id=2, bow=vec([7])); c.add(0, kf_id=3, bow=vec([9]))   # one-word vectors
    r, = c.reloc([vec([100, 200])], frame_ids=[2])            # a query sharing no word
    assert not r.sharing
    r, = c.reloc([vec([7])], frame_ids=[3])
    assert [k.mnId for _, k in r.score_and_match] == [1, 2]
    c.erase(1); c.erase(2); c.erase(3)
    r, = c.reloc([vec([7])], frame_ids=[4])                   # every entry erased
    assert not r.sharing
    # vectors longer than the LDS staging of the query (ORBX_KFDB_LDS_WORDS = 4096), among short ones
    rng = np.random.default_rng(12)
    c = make(dev_ex, 12, places=4, words=48, vocab=40000)
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


@pytest.mark.gpu
def test_thousands_of_entries(dev_ex):
    c = make(dev_ex, 13, places=40, words=40, vocab=8000)
    D.build_map(c, laps=3, per_place=25)                      # 3000 entries
    assert len(c.db) == 3000
    for _ in range(3):
        c.reloc([5, 17, 33], state=False)
    c.loop(20, same_place=True)
    for i in c.w.order[::7]:
        c.erase(i)
    c.reloc([1, 2], state=False)
    c.check_state()
    st = c.w.stats
    assert st["reloc_with_candidates"] == st["reloc"] and st["stale"] and st["unscored"]


@pytest.mark.gpu
def test_chain_from_descriptors(dev_ex):
    """descriptors -> orbx_bow_transform -> orbx_bow_vectors -> add / query: the database takes exactly what ComputeBoW yields"""
    from orb_slam2_detailed_comments_amd import ORBVocabulary
    from test_bow_transform import random_vocabulary
    rng = np.random.default_rng(14)
    voc_d, _ = random_vocabulary(rng, k=8, L=3, scoring=M.L1_NORM)
    voc = ORBVocabulary(dev_ex, **voc_d)
    db = KeyFrameDatabase(dev_ex, voc)
    assert db.scoring == M.L1_NORM
    w = D.World(14)
    w.model = M.KeyFrameDatabase(M.L1_NORM)
    c = D.Checked(w, db); w.covis = {}
    base = [rng.integers(0, 256, (300, 32), dtype=np.uint8) for _ in range(4)]

    def view(p):                                               # a place seen again: most descriptors kept, some bits flipped
        d = base[p].copy()
        flip = rng.random(d.shape) < 0.02
        d[flip] ^= np.uint8(1) << rng.integers(0, 8, size=int(flip.sum()), dtype=np.uint8)
        return voc.transform(d[rng.permutation(300)[:250]])[0]
    for i in range(12):
        c.add(i % 4, kf_id=i + 1, bow=view(i % 4))
    w.covis = {i: [j for j in range(1, 13) if j != i and (j - i) % 4 == 0] for i in range(1, 13)}
    rs = c.reloc([view(2), view(0)], frame_ids=[31, 32])
    assert all(r.candidates for r in rs)
    assert w.place_of[rs[0].candidates[0].mnId] == 2 and w.place_of[rs[1].candidates[0].mnId] == 0


@pytest.mark.gpu
def test_seeded_soak(dev_ex):
    c = make(dev_ex, 21, places=16, words=64, vocab=6000)
    D.assert_not_vacuous(D.play(c, 250, 2100))


# ------------------------------------------------------------------------------------------------ compat/KeyFrameDatabase.h
LIBDIR = os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "lib")
COMPAT = os.path.join(HERE, "compat_kfdb")


def _build_compat(out):
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", "-shared", "-fPIC", "-I" + COMPAT, "-I" + os.path.join(ROOT, "compat"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(COMPAT, "harness.cpp"), "-L" + LIBDIR, "-lorbx",
           "-Wl,-rpath," + LIBDIR, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


class CompatWorld:
    """the drop-in class behind its stand-ins (tests/compat_kfdb/harness.cpp) next to the model, on one seeded sequence"""

    def __init__(self, so, device, seed):
        import ctypes as C
        self.C, self.L = C, C.CDLL(so)
        self.L.kf_error.restype = C.c_char_p
        self.w = D.World(seed)
        self.ck(self.L.kf_reset(device, M.L1_NORM))
        self.all = {}            # every keyframe ever made, erased ones included (they keep their fields)

    def ck(self, rc):
        assert rc == 0, self.L.kf_error().decode()

    def _v(self, bow):
        w, v = np.ascontiguousarray(bow[0], np.uint32), np.ascontiguousarray(bow[1], np.float64)
        return w.ctypes.data_as(self.C.c_void_p), v.ctypes.data_as(self.C.c_void_p), len(w)

    def new(self, place, add=True):
        w = self.w
        i = w.next_kf; w.next_kf += 1
        bow = w.draw(place)
        kf = M.KeyFrame(i, bow)
        self.all[i] = kf
        self.ck(self.L.kf_new(self.C.c_long(i), *self._v(bow)))
        if add:
            self.add(i, place)
        return i

    def add(self, i, place):
        w = self.w
        w.model.add(self.all[i]); w.kfs[i] = self.all[i]; w.place_of[i] = place; w.order.append(i)
        self.ck(self.L.kf_add(self.C.c_long(i)))

    def erase(self, i):
        w = self.w
        w.model.erase(w.kfs.pop(i)); w.order.remove(i); del w.place_of[i]
        self.ck(self.L.kf_erase(self.C.c_long(i)))

    def graph(self, extra=()):
        C = self.C
        self.w.set_covisibility()
        for i in list(self.w.kfs) + list(extra):
            kf = self.all[i]
            conn = np.array([k.mnId for k in kf.connected], np.int64); ordd = np.array([k.mnId for k in kf.best_covis], np.int64)
            self.ck(self.L.kf_set_graph(C.c_long(i), conn.ctypes.data_as(C.c_void_p), len(conn), ordd.ctypes.data_as(C.c_void_p), len(ordd)))

    def _detect(self, call, res):
        C = self.C
        out = np.zeros(4096, np.int64); n = C.c_int(0); nu = C.c_int(0)
        self.ck(call(out.ctypes.data_as(C.c_void_p), 4096, C.byref(n), C.byref(nu)))
        assert list(out[:n.value]) == [k.mnId for k in res.candidates]
        assert nu.value == res.unscored_reads
        self.check_fields()

    def reloc(self, place):
        fid = self.w.next_frame; self.w.next_frame += 1
        F = M.Frame(fid, self.w.draw(place))
        self.graph()
        res = self.w.model.DetectRelocalizationCandidates(F)
        self._detect(lambda *a: self.L.kf_reloc(self.C.c_long(fid), *self._v(F.mBowVec), *a), res)
        return res

    def loop(self, place, min_score):
        i = self.new(place, add=False)
        cur = self.all[i]
        cur.connected = [self.w.kfs[j] for j in self.w.near(place)[-5:]]
        self.graph(extra=[i])
        res = self.w.model.DetectLoopCandidates(cur, min_score)
        self._detect(lambda *a: self.L.kf_loop(self.C.c_long(i), self.C.c_float(min_score), *a), res)
        self.add(i, place)
        return res

    def check_fields(self):
        C = self.C
        for i, kf in self.all.items():
            m = (C.c_long * 2)(); n = (C.c_int * 2)(); s = (C.c_float * 2)()
            self.ck(self.L.kf_fields(C.c_long(i), m, n, s))
            for f, loop in enumerate((False, True)):
                em, en, es, eok = kf.state(loop)
                assert (m[f], n[f]) == (em, en), (i, loop)
                if eok:
                    assert D.bits(s[f]) == D.bits(es), (i, loop)
                else:
                    assert np.isnan(s[f]), (i, loop)   # never scored: the shim leaves the member alone


def play_compat(so, device):
    cw = CompatWorld(so, device, 31)
    rng = np.random.default_rng(32)
    for _ in range(2):
        for p in range(cw.w.places):
            for _ in range(3):
                cw.new(p)
    rel = unscored = stale = loops = rejected = 0
    for _ in range(40):
        r = rng.random(); p = int(rng.integers(0, cw.w.places))
        if r < 0.5:
            res = cw.reloc(p)
            rel += 1; unscored += res.unscored_reads; stale += res.stale_reads
            assert res.candidates
        elif r < 0.8:
            res = cw.loop(p, 0.05 + 0.3 * rng.random())
            loops += 1; rejected += res.rejected_min_score
        elif r < 0.9:
            cw.erase(int(rng.choice(cw.w.order)))
        else:
            cw.new(p)
    assert rel and loops and unscored and stale and rejected
    cw.ck(cw.L.kf_clear())
    cw.w.model.clear(); cw.w.kfs.clear(); cw.w.order.clear(); cw.w.place_of.clear()
    assert not cw.reloc(0).sharing
    cw.ck(cw.L.kf_reset(-2, M.L1_NORM))   # the device database goes while the runtime is up, not at process exit


def test_compat_header_compiles_and_runs_on_the_host_path(built_lib, tmp_path):
    import shutil
    assert shutil.which("g++")
    so = str(tmp_path / "kfdb_compat.so")
    p = _build_compat(so)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]
    play_compat(so, -2)


@pytest.mark.gpu
def test_compat_class_through_stand_ins_on_the_device(built_lib, tmp_path):
    so = str(tmp_path / "kfdb_compat.so")
    p = _build_compat(so)
    assert p.returncode == 0, p.stderr[-4000:]
    play_compat(so, 0)


# ------------------------------------------------------------------------------------------------ the code object
def test_kernels_have_no_scratch_and_round_divide_and_square_root(built_lib):
    """chi-square and Bhattacharyya / L2 on the device rest on correctly rounded FP64 division and square root: the score
    kernels must hold the full division sequence (scale, reciprocal estimate, fused corrections, fixup), not a bare reciprocal,
    and the refined square root (reciprocal square root estimate + fused corrections), not a bare v_sqrt_f64 (about 2^-29
    relative accuracy on its own).  The bitwise GPU comparison against orbx_bow_score is the functional check."""
    import re
    from test_pipeline_room import _kernel_metadata
    from test_abi import _device_disassembly
    meta = _kernel_metadata(built_lib)
    names = [k for k in meta if "k_kfdb" in k]
    assert len(names) == 3, names
    for k in names:
        assert int(meta[k]["private_segment_fixed_size"]) == 0, k
    asm = _device_disassembly(built_lib)
    for kern in ("k_kfdb_score", "k_kfdb_score_slots"):
        m = re.search(r"<_Z\d+%s[^>]*>:\n(.*?)s_endpgm" % kern, asm, re.S)
        assert m, kern
        body = m.group(1)
        for op in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64", "v_rsq_f64", "v_fma_f64"):
            assert op in body, (kern, op)
        assert "v_sqrt_f64" not in body and "v_rcp_f32" not in body, kern
