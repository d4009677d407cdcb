"""Batched SearchByBoW (orbx_search_by_bow_keyframe_frame_batch / orbx_search_by_bow_keyframes_batch): the candidate loops of
Tracking::Relocalization (src/Tracking.cc:2283-2300) and LoopClosing::ComputeSim3 (src/LoopClosing.cc:440-466) as one call,
with the selection on the device (k_bow_select, one wave per common vocabulary node; k_bow_rot, one workgroup per problem).

CPU part: the ABI (symbols, validation before any device work on a host-only handle), the code object (no scratch in the new
kernels) and the compat shim's two overloads.  GPU part: every batched problem equals the C oracle and the existing single
call, on extracted keypoints and on adversarial inputs, plus a seeded soak.  The vocabulary is synthetic (make_featvec: node =
a few descriptor bits; ORBvoc.txt is not in the image); the policies only read node ids."""
import ctypes as C
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import oracle
from orb_slam2_detailed_comments_amd import ORBextractor, ORBmatcher, OrbxError, _capi
from test_bow_policies import make_featvec, random_kf, perturbed_copy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "compat_stubs")
NAMES = ("orbx_search_by_bow_keyframe_frame_batch", "orbx_search_by_bow_keyframes_batch")


# ----------------------------------------------------------------------------------------------- CPU
def test_symbols_declared_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "orbx.h")).read()
    L = _capi.lib()
    for name in NAMES:
        assert f"orbx_status {name}(" in header
        assert name in _capi.SYMBOLS
        assert hasattr(L, name)


def _host_only_matcher():
    return ORBmatcher(0.75, True, extractor=ORBextractor(1000, 1.2, 8, 20, 7, device=-2))


def _cpu_inputs(seed=0, n=200):
    rng = np.random.default_rng(seed)
    kf = random_kf(rng, n)
    f = perturbed_copy(rng, kf)
    kf["feat_vec"] = make_featvec(kf["desc"], shuffle_rng=rng)
    f["feat_vec"] = make_featvec(f["desc"], shuffle_rng=rng)
    return kf, f


def _flat(fv):
    nodes = sorted(fv)
    begin = np.cumsum([0] + [len(fv[k]) for k in nodes]).astype(np.int32)
    return np.array(nodes, np.uint32), begin, np.array([j for k in nodes for j in fv[k]], np.uint32)


def _status(fn):
    with pytest.raises(OrbxError) as e:
        fn()
    return e.value.status


def test_host_only_validation(built_lib):
    m = _host_only_matcher()
    kf, f = _cpu_inputs()
    fk, fd = f["keys_un"], f["desc"]
    # a duplicated feature index (the same feature under two nodes)
    node, begin, index = _flat(kf["feat_vec"])
    dup = index.copy(); dup[1] = dup[0]
    kf_dup = dict(kf, feat_vec=(node, begin, dup))
    # node ids out of order
    unsorted = node.copy(); unsorted[[0, 1]] = unsorted[[1, 0]]
    kf_unsorted = dict(kf, feat_vec=(unsorted, begin, index))
    # an index >= n
    big = index.copy(); big[-1] = len(kf["desc"])
    kf_big = dict(kf, feat_vec=(node, begin, big))
    for bad in (kf_dup, kf_unsorted, kf_big):
        assert _status(lambda: m.SearchByBoWBatch([kf, bad], fk, fd, f["feat_vec"])) == _capi.BAD_ARGUMENT
        assert _status(lambda: m.SearchByBoWKeyFramesBatch(kf, [dict(f, feat_vec=kf["feat_vec"]), bad])) == _capi.BAD_ARGUMENT
        assert _status(lambda: m.SearchByBoWKeyFramesBatch(bad, [f])) == _capi.BAD_ARGUMENT
        assert _status(lambda: m.SearchByBoWBatch([f], bad["keys_un"], bad["desc"], bad["feat_vec"])) == _capi.BAD_ARGUMENT
    # the single calls keep accepting repeated indices (their sequential walk handles them): still NO_DEVICE here
    assert _status(lambda: m.SearchByBoW(kf_dup, fk, fd, f["feat_vec"])) == _capi.NO_DEVICE
    # well-formed input reaches the device step
    assert _status(lambda: m.SearchByBoWBatch([kf, kf], fk, fd, f["feat_vec"])) == _capi.NO_DEVICE
    assert _status(lambda: m.SearchByBoWKeyFramesBatch(kf, [f, f])) == _capi.NO_DEVICE
    # nothing to do: empty lists
    assert m.SearchByBoWBatch([], fk, fd, f["feat_vec"]) == []
    assert m.SearchByBoWKeyFramesBatch(kf, []) == []


def test_host_only_raw_arguments(built_lib):
    L = _capi.lib()
    m = _host_only_matcher()
    h = m._ex.handle
    kf, f = _cpu_inputs(1)
    keep = []
    kv, fv = m._kf_view(kf, keep), m._featvec(f["feat_vec"], keep)
    fk, fd = np.ascontiguousarray(f["keys_un"], _capi.KP_DTYPE), np.ascontiguousarray(f["desc"], np.uint8)
    out = np.full(max(len(fk), len(kf["desc"])), -1, np.int32)
    oarr = (C.c_void_p * 2)(out.ctypes.data, out.ctypes.data)
    n = (C.c_int * 2)()
    views = (C.c_void_p * 2)(C.addressof(kv), C.addressof(kv))
    null_view = (C.c_void_p * 2)(C.addressof(kv), None)
    ff = lambda K, arr: L.orbx_search_by_bow_keyframe_frame_batch(h, K, arr, _capi.ptr(fk), _capi.ptr(fd), len(fk), C.byref(fv),
                                                                  0.75, 1, oarr, n)
    kk = lambda K, arr: L.orbx_search_by_bow_keyframes_batch(h, C.byref(kv), K, arr, 0.75, 1, oarr, n)
    for fn in (ff, kk):
        assert fn(-1, views) == _capi.BAD_ARGUMENT
        assert fn(2, null_view) == _capi.BAD_ARGUMENT
        assert fn(0, None) == _capi.OK
        assert fn(2, views) == _capi.NO_DEVICE


def test_new_kernels_use_no_scratch(built_lib):
    from test_pipeline_room import _kernel_metadata
    meta = _kernel_metadata(built_lib)
    for name in ("k_bow_select", "k_bow_rot"):
        hits = [v for k, v in meta.items() if name in k]
        assert len(hits) == 2, (name, [k for k in meta if "bow" in k])   # the KF <-> F and KF <-> KF instances
        for v in hits:
            assert int(v["private_segment_fixed_size"]) == 0, v["name"]


def test_shim_bow_batch_parses_and_type_checks():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    p = subprocess.run([gxx, "-std=c++14", "-Wall", "-fsyntax-only", "-I" + STUBS, "-I" + os.path.join(ROOT, "compat"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(STUBS, "driver_bow_batch.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]


# ----------------------------------------------------------------------------------------------- GPU
def _check_kf_frame(m, kfs, fk, fd, ffv, ratio, ori, single=True):
    res = m.SearchByBoWBatch(kfs, fk, fd, ffv)
    assert len(res) == len(kfs)
    for k, (n, out) in enumerate(res):
        on, oout = oracle.search_by_bow_kf_frame(kfs[k], fk, fd, ffv, ratio, ori)
        assert n == on and np.array_equal(out, oout), (k, n, on)
        if single:
            sn, sout = m.SearchByBoW(kfs[k], fk, fd, ffv)
            assert n == sn and np.array_equal(out, sout), (k, n, sn)
    return [n for n, _ in res]


def _check_kf_kf(m, kf1, kf2s, ratio, ori, single=True):
    res = m.SearchByBoWKeyFramesBatch(kf1, kf2s)
    assert len(res) == len(kf2s)
    for k, (n, out) in enumerate(res):
        on, oout = oracle.search_by_bow_kf_kf(kf1, kf2s[k], ratio, ori)
        assert n == on and np.array_equal(out, oout), (k, n, on)
        if single:
            sn, sout = m.SearchByBoWKeyFrames(kf1, kf2s[k])
            assert n == sn and np.array_equal(out, sout), (k, n, sn)
    return [n for n, _ in res]


@pytest.fixture(scope="module")
def stream_keyframes():
    from orb_slam2_detailed_comments_amd import synth
    frames = synth.stream(640, 480, 16, stream_id=51)
    ex = ORBextractor(1000, max_batch=16)
    res = ex.extract_batch(frames)
    rng = np.random.default_rng(7)
    kfs = [dict(keys_un=k, desc=d, has_map_point=(rng.uniform(size=len(k)) < 0.7).astype(np.uint8),
                feat_vec=make_featvec(d, bits=7, shuffle_rng=rng)) for k, d in res]
    return ex, kfs


@pytest.mark.gpu
def test_gpu_batch_equals_oracle_and_single_calls(stream_keyframes):
    ex, kfs = stream_keyframes
    F = kfs[0]
    best = 0
    for ratio, ori in ((0.7, True), (0.75, False)):
        m = ORBmatcher(ratio, ori, extractor=ex)
        for K in (1, 5, 15):
            n1 = _check_kf_frame(m, kfs[1:1 + K], F["keys_un"], F["desc"], F["feat_vec"], ratio, ori)
            n2 = _check_kf_kf(m, F, kfs[1:1 + K], ratio, ori)
            best = max(best, min(n1), min(n2))
    assert best > 30   # not vacuous: some setting matches more than 30 features in every problem


@pytest.mark.gpu
@pytest.mark.parametrize("ori", [True, False])
def test_gpu_wide_nodes(ori):
    """bits=1: two nodes of ~500 features, rows and columns far beyond one wave"""
    rng = np.random.default_rng(21)
    kf = random_kf(rng, 1000, p_mp=0.8)
    fs = [perturbed_copy(rng, kf, nflip=10, drop=0.1) for _ in range(3)]
    kf["feat_vec"] = make_featvec(kf["desc"], bits=1, shuffle_rng=rng)
    for f in fs:
        f["feat_vec"] = make_featvec(f["desc"], bits=1, shuffle_rng=rng)
    assert max(len(v) for v in kf["feat_vec"].values()) > 300
    m = ORBmatcher(0.8, ori, extractor=ORBextractor(1000))
    n = _check_kf_frame(m, [f for f in fs], kf["keys_un"], kf["desc"], kf["feat_vec"], 0.8, ori)
    n2 = _check_kf_kf(m, kf, fs, 0.8, ori)
    assert min(n) > 30 and min(n2) > 30


@pytest.mark.gpu
def test_gpu_exact_ties():
    """duplicated and one-bit-perturbed descriptors: many equal distances; the first in visiting order must win"""
    rng = np.random.default_rng(22)
    base = random_kf(rng, 300, p_mp=0.9)
    d = base["desc"]
    flip = d.copy(); flip[:, 5] ^= np.uint8(1)                     # byte 5: the node (bytes 0, 7) stays the same
    desc = np.concatenate([d, flip, d, d])
    keys = np.concatenate([base["keys_un"]] * 4)
    f = dict(keys_un=keys, desc=desc, has_map_point=np.ones(len(desc), np.uint8))
    f["feat_vec"] = make_featvec(desc, bits=4, shuffle_rng=rng)
    kf = dict(base, desc=np.concatenate([d, flip]), keys_un=np.concatenate([base["keys_un"]] * 2),
              has_map_point=np.ones(600, np.uint8))
    kf["feat_vec"] = make_featvec(kf["desc"], bits=4, shuffle_rng=rng)
    for ratio, ori in ((1.0, False), (1.0, True), (0.9, False)):
        m = ORBmatcher(ratio, ori, extractor=ORBextractor(1000))
        _check_kf_frame(m, [kf, kf], f["keys_un"], f["desc"], f["feat_vec"], ratio, ori)
        _check_kf_kf(m, kf, [f, f], ratio, ori)
        _check_kf_kf(m, f, [kf], ratio, ori)


@pytest.mark.gpu
def test_gpu_degenerate_problems():
    """all has_map_point zero, a candidate with n == 0, one with an empty feature vector, the same candidate twice, nnratio 1"""
    rng = np.random.default_rng(23)
    kf = random_kf(rng, 500)
    kf["feat_vec"] = make_featvec(kf["desc"], shuffle_rng=rng)
    f = perturbed_copy(rng, kf)
    f["feat_vec"] = make_featvec(f["desc"], shuffle_rng=rng)
    no_mp = dict(f, has_map_point=np.zeros(len(f["desc"]), np.uint8))
    empty = dict(keys_un=kf["keys_un"][:0], desc=kf["desc"][:0], has_map_point=kf["has_map_point"][:0], feat_vec={})
    no_fv = dict(f, feat_vec={})
    cands = [f, no_mp, empty, no_fv, f, f]
    for ratio, ori in ((1.0, True), (0.75, True), (0.6, False)):
        m = ORBmatcher(ratio, ori, extractor=ORBextractor(1000))
        n = _check_kf_frame(m, cands, kf["keys_un"], kf["desc"], kf["feat_vec"], ratio, ori)
        assert n[1] == n[2] == n[3] == 0 and n[0] == n[4] == n[5] > 0
        n2 = _check_kf_kf(m, kf, cands, ratio, ori)
        assert n2[1] == n2[2] == n2[3] == 0 and n2[0] == n2[4] == n2[5] > 0
        # the shared side empty, or without MapPoints
        _check_kf_frame(m, cands, empty["keys_un"], empty["desc"], {}, ratio, ori)
        _check_kf_kf(m, dict(kf, has_map_point=np.zeros(500, np.uint8)), cands, ratio, ori)
        _check_kf_kf(m, empty, cands, ratio, ori)


@pytest.mark.gpu
def test_gpu_rotation_histogram_shapes():
    """angle patterns that fill one or two bins, and ones where the 0.1 * max1 rule drops the second and third bins"""
    rng = np.random.default_rng(24)
    kf = random_kf(rng, 800, p_mp=0.9)
    kf["feat_vec"] = make_featvec(kf["desc"], shuffle_rng=rng)
    f = perturbed_copy(rng, kf, nflip=6, drop=0.05)
    f["feat_vec"] = make_featvec(f["desc"], shuffle_rng=rng)
    kf["keys_un"] = kf["keys_un"].copy(); kf["keys_un"]["angle"] = 0.0
    nf = len(f["desc"])
    patterns = {
        "one bin": np.zeros(nf, np.float32),
        "two bins": np.where(np.arange(nf) % 2 == 0, 0.0, 36.0).astype(np.float32),
        "minor bins dropped": np.select([np.arange(nf) % 40 == 0, np.arange(nf) % 40 == 1], [36.0, 72.0], 0.0).astype(np.float32),
        "third dropped": np.select([np.arange(nf) % 40 == 0, np.arange(nf) % 4 == 1], [72.0, 36.0], 0.0).astype(np.float32),
        "bin 30 wraps to 0": np.where(np.arange(nf) % 3 == 0, 359.0, 0.5).astype(np.float32),
    }
    m = ORBmatcher(0.9, True, extractor=ORBextractor(1000))
    m_no = ORBmatcher(0.9, False, extractor=ORBextractor(1000))
    dropped = 0
    for name, ang in patterns.items():
        fp = dict(f, keys_un=f["keys_un"].copy()); fp["keys_un"]["angle"] = ang
        n = _check_kf_frame(m, [kf, kf], fp["keys_un"], fp["desc"], fp["feat_vec"], 0.9, True)
        n2 = _check_kf_kf(m, fp, [kf], 0.9, True)
        n_no = _check_kf_frame(m_no, [kf], fp["keys_un"], fp["desc"], fp["feat_vec"], 0.9, False)
        assert n[0] > 30 and n2[0] > 30, name
        dropped += n_no[0] - n[0]
    assert dropped > 0   # the rule removed matches in at least one pattern


@pytest.mark.gpu
def test_gpu_soak_random_shapes():
    """seeded random shapes, K, ratios and feature-vector granularities, 60 s at most: zero differences from the oracle"""
    rng = np.random.default_rng(2024)
    ex = ORBextractor(1000)
    t0, problems = time.time(), 0
    while time.time() - t0 < 45 and problems < 4000:
        n1 = int(rng.integers(0, 1500))
        bits = int(rng.integers(1, 9))
        K = int(rng.integers(1, 21))
        ratio = float(rng.choice([0.6, 0.7, 0.75, 0.8, 0.9, 1.0]))
        ori = bool(rng.integers(0, 2))
        base = random_kf(rng, n1, p_mp=float(rng.uniform(0, 1)))
        base["feat_vec"] = make_featvec(base["desc"], bits=bits, shuffle_rng=rng)
        cands = []
        for _ in range(K):
            c = perturbed_copy(rng, base, nflip=int(rng.integers(0, 30)), drop=float(rng.uniform(0, 0.6)))
            c["feat_vec"] = make_featvec(c["desc"], bits=bits, shuffle_rng=rng)
            cands.append(c)
        m = ORBmatcher(ratio, ori, extractor=ex)
        _check_kf_frame(m, cands, base["keys_un"], base["desc"], base["feat_vec"], ratio, ori, single=False)
        _check_kf_kf(m, base, cands, ratio, ori, single=False)
        problems += 2 * K
    assert problems > 100
