"""Batched MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (orbx_distinctive_descriptors_batch[_device],
orbx_update_normal_and_depth_batch), the part that needs no GPU: tests/mappoint_model.py against the reference's compiled
src/MapPoint.cc (oracle/_ref/libref_matcher_{strict,fma}.so; tests/golden/mappoint_batch_*.json where they cannot be built) for
the descriptor, against the C++ restatement of tests/compat_mappoint/ for normal and depth, the ABI, validation before any
device work on a host-only handle, no scratch and the rounded divide / square root in the new kernels, and the HIP-free planning
and packing unit under AddressSanitizer + UndefinedBehaviorSanitizer (tests/san_mappoint_pack.cpp, a stand-alone program).

What the compiled harness cannot show: its KeyFrame::isBad() is constant false, so a bad keyframe is played into it as the
observation left out -- which is what the caller-side snapshot hands to the batch; the filter itself runs in
tests/test_compat_mappoint.py.  UpdateNormalAndDepth has no export there: it is pinned to the stand-in's stated arithmetic only."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import mappoint_harness as mh
import mappoint_model as mm
from compat_scenes import KP, Scene
from orb_slam2_detailed_comments_amd import ORBextractor, OrbxError, _capi, mappoint
from test_ref_matcher import VARIANTS, ref_harness, reference_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mappoint_batch_%s.json")
NAMES = ("orbx_distinctive_descriptors_batch", "orbx_distinctive_descriptors_batch_device", "orbx_update_normal_and_depth_batch")
KERNELS = {"k_mp_distinct": 2, "k_mp_normal_depth": 1}   # instances in the code object (k_mp_distinct and k_mp_distinct_wide)
PREFILL = np.full(32, 0x5A, np.uint8)
SCENE_SEED = 7


def golden_scene():
    """the scene of the records and of tests/test_mappoint_batch_gpu.py with the model's answer (computed once per process)"""
    if "s" not in _CACHE:
        ob, desc = mm.scene(SCENE_SEED)
        _CACHE["s"] = (ob, desc) + mm.distinct_batch(ob, desc, np.tile(PREFILL, (len(ob) - 1, 1)))
    return _CACHE["s"]


_CACHE = {}


def record(best_idx, best_median, best_desc):
    return dict(best_idx=[int(v) for v in best_idx], best_median=[int(v) for v in best_median], desc_sha256=mm.desc_hash(best_desc))


# ----------------------------------------------------------------------------------------------- the compiled reference
def ref_state(H, p, cap=512):
    bad, nobs, ne = (np.zeros(1, np.int32) for _ in range(3))
    d, ok, oi = np.zeros(32, np.uint8), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    H("h_mp_state", p, bad, nobs, d, ok, oi, cap, ne)
    assert ne[0] <= cap
    return d, list(zip(ok[:ne[0]].tolist(), oi[:ne[0]].tolist()))


def play_reference(H, obs_begin, desc, seed=3, bad_points=()):
    """row r of point p lives in keyframe r, slot p; the observations are added in a shuffled order.  Returns the descriptor the
    reference leaves on every point and the rows of every point in the order the reference's map reports."""
    rng = np.random.default_rng(seed)
    P = len(obs_begin) - 1
    n = np.diff(obs_begin)
    kd = np.zeros((max(int(n.max()), 1), P, 32), np.uint8)
    for p in range(P):
        kd[:n[p], p] = desc[obs_begin[p]:obs_begin[p + 1]]
    S = Scene(H)
    for k in range(len(kd)):
        S.kf(np.zeros(P, KP), kd[k])
    for p in range(P):
        S.mp(PREFILL)
        for k in rng.permutation(int(n[p])):
            S.observe(p, int(k), p)
    for p in bad_points:
        H("h_set_bad", p)
    out, rows = [], []
    for p in range(P):
        order = ref_state(H, p)[1]
        H("h_compute_descriptor", p)
        out.append(ref_state(H, p)[0])
        rows.append(np.stack([kd[k, i] for k, i in order]) if order else np.zeros((0, 32), np.uint8))
    return np.stack(out), rows


@pytest.mark.parametrize("variant", VARIANTS)
def test_model_equals_compiled_mappoint_and_records(variant):
    ob, desc, idx, med, best = golden_scene()
    gold = json.load(open(GOLDEN % variant))
    assert record(idx, med, best) == gold
    if not reference_available():
        return                                                       # the records stand for the compiled reference
    out, rows = play_reference(ref_harness(variant), ob, desc)
    for p in range(len(ob) - 1):                                     # the model is fed the order the reference reports
        i, m, _ = mm.distinct_one(rows[p])
        want = rows[p][i] if len(rows[p]) else PREFILL
        assert np.array_equal(out[p], want), ("point", p, len(rows[p]))
        assert np.array_equal(rows[p], desc[ob[p]:ob[p + 1]]), "keyframes are kept in id order by this harness"
        assert (i, m) == (idx[p], med[p])
    assert mm.desc_hash(out) == gold["desc_sha256"]


def test_scene_plants_what_it_claims():
    """on the model's side: ties between different descriptors in every size class above 3, a best row that is not row 0,
    best_idx == 0 for N <= 2, medians of N <= 2 are 0, the N == 3 rule, duplicate rows, points without rows at both ends"""
    ob, desc, idx, med, best = golden_scene()
    n = np.diff(ob)
    assert n[0] == 0 and n[-1] == 0 and (n[1:-1] == 0).any()
    assert set(mm.SIZES) <= set(n.tolist())
    tie_sizes, dup = set(), False
    for p in range(len(n)):
        rows = desc[ob[p]:ob[p + 1]]
        if n[p] == 0:
            assert idx[p] == -1 and med[p] == -1 and np.array_equal(best[p], PREFILL)
            continue
        _, m, meds = mm.distinct_one(rows)
        if n[p] <= 2:
            assert idx[p] == 0 and (meds == 0).all()
        if n[p] == 3:
            D = mm.distance_matrix(rows)
            assert all(meds[i] == min(D[i][j] for j in range(3) if j != i) for i in range(3))
        winners = [i for i in range(n[p]) if meds[i] == m]
        if len({rows[i].tobytes() for i in winners}) > 1:
            tie_sizes.add(int(n[p]))
        dup |= n[p] > 3 and len({r.tobytes() for r in rows}) < n[p]
    assert tie_sizes >= {s for s in mm.SIZES if s > 3}, tie_sizes
    assert (idx > 0).any() and dup


@pytest.mark.parametrize("variant", VARIANTS)
def test_order_is_part_of_the_contract(variant):
    """two different rows with equal medians: the first in the MAP's order wins, so the reversed order gives another
    descriptor; a point set bad, and a point whose bad keyframe's observation the snapshot leaves out"""
    rng = np.random.default_rng(5)
    a, b, c = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    pts = [np.stack([a, b]), np.stack([a, b, c, mm.flip(rng, c, 2)]), np.stack([b, c, a])]
    ob = np.concatenate([[0], np.cumsum([len(x) for x in pts])]).astype(np.int32)
    desc = np.concatenate(pts)
    assert not np.array_equal(mm.distinct_batch(ob[:2], pts[0])[2], mm.distinct_batch(ob[:2], pts[0][::-1])[2])
    if not reference_available():
        return                                                       # no harness to ask for its order
    out, rows = play_reference(ref_harness(variant), ob, desc, bad_points=(1,))
    assert np.array_equal(out[0], rows[0][mm.distinct_one(rows[0])[0]])
    assert not np.array_equal(out[0], rows[0][::-1][mm.distinct_one(rows[0][::-1])[0]])
    assert np.array_equal(out[1], PREFILL) and len(rows[1]) == 0    # SetBadFlag: the descriptor comes out unchanged
    # keyframe 2 bad: the snapshot hands rows 0 and 1 of point 2 to the batch; the reference is played that point without it
    snap = pts[2][:2]
    out2, rows2 = play_reference(ref_harness(variant), np.array([0, 2], np.int32), snap)
    assert np.array_equal(out2[0], mm.distinct_batch([0, 2], rows2[0])[2][0])


# ----------------------------------------------------------------------------------------------- normal and depth
@pytest.fixture(scope="module")
def stand_in(built_lib, tmp_path_factory):
    assert shutil.which("g++")
    return mh.build(str(tmp_path_factory.mktemp("compat_mappoint") / "harness.so"))


def test_model_equals_stand_in_single_calls(stand_in):
    """random float positions and centres (no dyadic values: every rounding step counts): the model is bit-equal to the C++
    restatement over the cv::Mat stand-in, descriptors included, in the map's own order"""
    pts, kfs, order = mh.play_scene(stand_in)
    stand_in.call("mpt_single_loop", order, len(order), 1, 1)
    d, out = stand_in.states(len(pts))
    md, mout = mh.model_scene(stand_in, pts, kfs)
    assert np.array_equal(d, md)
    assert np.array_equal(out.view(np.uint32), mout.view(np.uint32))
    for p in (5, 7, 9):                                              # unobserved, bad, observed by a bad keyframe alone
        assert np.array_equal(d[p], pts[p]["desc"])
    assert np.array_equal(out[5], np.concatenate([pts[5]["normal"], [pts[5]["dmin"], pts[5]["dmax"]]]))
    assert not np.array_equal(out[9, :3], pts[9]["normal"])          # ... whose normal is still refreshed


# ----------------------------------------------------------------------------------------------- ABI
def test_symbols_declared_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "orbx.h")).read()
    L = _capi.lib()
    for name in NAMES:
        assert f"orbx_status {name}(" in header
        assert name in _capi.SYMBOLS
        assert hasattr(L, name)
    assert L.orbx_abi_version() == 1


def test_new_kernels_use_no_scratch_and_round_divide_and_square_root(built_lib):
    import re
    from test_abi import _device_disassembly
    from test_pipeline_room import _kernel_metadata
    meta = _kernel_metadata(built_lib)
    for name, count in KERNELS.items():
        hits = [v for k, v in meta.items() if name in k]
        assert len(hits) == count, (name, [k for k in meta if "k_mp" in k])
        for v in hits:
            assert int(v["private_segment_fixed_size"]) == 0, v["name"]
    m = re.search(r"<_Z\d+k_mp_normal_depth[^>]*>:\n(.*?)s_endpgm", _device_disassembly(built_lib), re.S)
    assert m
    body = m.group(1)
    # the full double division and the refined double square root, and the full float division of mfMinDistance
    for op in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64", "v_rsq_f64", "v_fma_f64", "v_div_fixup_f32"):
        assert op in body, op
    assert "v_sqrt_f64" not in body


# ----------------------------------------------------------------------------------------------- validation
def _status(fn):
    with pytest.raises(OrbxError) as e:
        fn()
    return e.value.status


def test_host_only_validation(built_lib):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    L, h, P = _capi.lib(), ex.handle, _capi.ptr
    B, ND, OK = _capi.BAD_ARGUMENT, _capi.NO_DEVICE, _capi.OK
    ob = np.array([0, 2, 2, 5], np.int32)
    desc = np.zeros((5, 32), np.uint8)
    rows = np.array([0, 1, 2, 3, 9], np.int64)
    idx, med, out = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros((3, 32), np.uint8)
    dd = lambda n=3, b=ob, d=desc, i=idx, m=med, o=out: L.orbx_distinctive_descriptors_batch(h, n, P(b), P(d), P(i), P(m), P(o))
    assert dd() == ND
    assert dd(m=None, o=None) == ND
    assert dd(n=0) == OK and dd(n=0, b=None, d=None, i=None) == OK
    assert dd(n=-1) == B and dd(b=None) == B and dd(d=None) == B and dd(i=None) == B
    assert dd(b=np.array([0, 3, 2, 5], np.int32)) == B and dd(b=np.array([1, 2, 2, 5], np.int32)) == B
    assert dd(b=np.zeros(4, np.int32), d=None) == ND                 # no rows at all: nothing to read
    pool = 0x10000
    dv = lambda n=3, b=ob, pl=pool, pr=10, r=rows, i=idx: L.orbx_distinctive_descriptors_batch_device(h, P(pl), pr, n, P(b), P(r), P(i),
                                                                                                   P(med), P(out))
    assert dv() == ND
    assert dv(n=0) == OK
    assert dv(pr=9) == B and dv(pr=-1) == B and dv(n=-1) == B       # row 9 of a pool of 9
    assert dv(r=np.array([0, 1, -1, 3, 4], np.int64)) == B
    assert dv(pl=None) == B and dv(r=None) == B and dv(i=None) == B and dv(pl=pool + 4) == B
    assert dv(b=np.array([0, 2, 1, 5], np.int32)) == B
    f3, c, o1 = np.zeros((3, 3), np.float32), np.zeros((5, 3), np.float32), np.zeros(3, np.float32)
    lvl = np.array([0, 99, 7], np.int32)                             # point 1 has no rows: its level is not looked at
    nd = lambda n=3, b=ob, p=f3, cc=c, r=f3, l=lvl, nn=f3, a=o1, z=o1: L.orbx_update_normal_and_depth_batch(
        h, n, P(b), P(p), P(cc), P(r), P(l), P(nn), P(a), P(z))
    assert nd() == ND
    assert nd(n=0) == OK and nd(n=-1) == B
    assert nd(l=np.array([0, 0, 8], np.int32)) == B and nd(l=np.array([-1, 0, 0], np.int32)) == B
    for k in ("b", "p", "cc", "r", "l", "nn", "a", "z"):
        assert nd(**{k: None}) == B, k
    assert nd(b=np.array([0, 3, 2, 5], np.int32)) == B
    assert L.orbx_update_normal_and_depth_batch(None, 0, None, None, None, None, None, None, None, None) == B
    assert L.orbx_distinctive_descriptors_batch(None, 0, None, None, None, None, None) == B
    # the Python mirror raises what the C call returns
    assert _status(lambda: mappoint.distinctive_descriptors_batch(ex, ob, desc)) == ND
    assert _status(lambda: mappoint.distinctive_descriptors_batch_device(ex, pool, 9, ob, rows)) == B
    assert _status(lambda: mappoint.update_normal_and_depth_batch(ex, ob, f3, c, f3, np.array([0, 0, 8]))) == B
    i0, m0, o0 = mappoint.distinctive_descriptors_batch(ex, np.zeros(1, np.int32), np.zeros((0, 32), np.uint8))
    assert len(i0) == 0 and len(m0) == 0 and o0.shape == (0, 32)


# ----------------------------------------------------------------------------------------------- sanitizers
def test_packing_unit_clean_under_asan_ubsan(tmp_path):
    """csrc/orbx_mappoint.cpp (validation, size-class plan, packing, scatter; HIP-free) built with g++
    -fsanitize=address,undefined together with tests/san_mappoint_pack.cpp: points without rows at the front, in the middle and
    at the end, every size-class boundary, one point with 300 rows, every rejection, random ragged batches"""
    exe = str(tmp_path / "san_mappoint_pack")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_mappoint_pack.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_mappoint.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr


def test_compat_body_compiles_without_warnings():
    """compat/MapPoint_batch.inl through the stand-ins, syntax only (no library, no GPU)"""
    assert shutil.which("g++")
    p = subprocess.run(mh.build_cmd(None, syntax_only=True), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]
