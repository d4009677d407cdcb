"""Batched device-resident SearchByProjection of the two tracking matchers (orbx_search_by_projection_frame_batch_device /
orbx_search_by_projection_mappoints_batch_device), the part that needs no GPU: the two-phase selection scheme against the C
oracle (tests/track_model.py), the ABI, validation before any device work on a host-only handle, no scratch in the new kernels,
and the HIP-free packing unit under AddressSanitizer + UndefinedBehaviorSanitizer (tests/san_track_pack.cpp, a stand-alone
program)."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import track_model as tm
from orb_slam2_detailed_comments_amd import ORBextractor, ORBmatcher, OrbxError, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orbx_search_by_projection_frame_batch_device", "orbx_search_by_projection_mappoints_batch_device")
KERNELS = {"k_track_project": 1, "k_track_cand": 2, "k_track_select": 2}   # instances in the code object


# ----------------------------------------------------------------------------------------------- the scheme
def test_two_phase_model_equals_oracle_frame_policy():
    """>= 100 seeded, conflict-heavy scenes: 'unconstrained in parallel, ordered pass rescans only on conflict' gives what the
    sequential reference gives, and the scenes do make the ordered pass rescan, override and drop events"""
    scale = tm.scale_factors()
    tot = dict(rescans=0, overrides=0, dropped_events=0, kept_overridden=0, live=0)
    for seed in range(120):
        rng = np.random.default_rng(1000 + seed)
        frame = tm.make_frame(rng, int(rng.integers(1, 301)))
        p = tm.make_ff_problem(rng, frame, int(rng.integers(1, 401)), motion=("side", "forward", "backward")[seed % 3],
                               th=(7.0, 15.0, 30.0)[seed % 3], mono=int(seed % 5 == 0), scale=scale)
        ori = seed % 4 != 0
        on, om = tm.oracle_ff(frame, p, ori, oracle.FP_STRICT, scale)
        n, m, st = tm.model_ff(frame, p, ori, scale)
        assert n == on and np.array_equal(m, om), f"seed {seed}"
        for k in tot:
            tot[k] += st[k]
    assert tot["rescans"] > 0 and tot["overrides"] > 0 and tot["dropped_events"] > 0 and tot["kept_overridden"] > 0, tot
    assert tot["live"] > 1000


def test_two_phase_model_equals_oracle_mappoint_policy():
    scale = tm.scale_factors()
    tot = dict(rescans=0, live=0, ratio_rejects=0)
    for seed in range(120):
        rng = np.random.default_rng(2000 + seed)
        frame = tm.make_frame(rng, int(rng.integers(1, 301)))
        p = tm.make_mp_problem(rng, frame, int(rng.integers(1, 401)), th=(1.0, 3.0, 5.0)[seed % 3])
        ratio = (0.6, 0.8, 1.0)[(seed // 3) % 3]
        on, oa = tm.oracle_mp(frame, p, ratio, scale)
        n, a, st = tm.model_mp(frame, p, ratio, scale)
        assert n == on and np.array_equal(a, oa), f"seed {seed}"
        for k in tot:
            tot[k] += st[k]
    assert tot["rescans"] > 0 and tot["ratio_rejects"] > 0 and tot["live"] > 1000, tot


# ----------------------------------------------------------------------------------------------- ABI
def test_symbols_declared_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "orbx.h")).read()
    L = _capi.lib()
    for name in NAMES:
        assert f"orbx_status {name}(" in header
        assert name in _capi.SYMBOLS
        assert hasattr(L, name)
    assert L.orbx_abi_version() == 1


def test_new_kernels_use_no_scratch(built_lib):
    from test_pipeline_room import _kernel_metadata
    meta = _kernel_metadata(built_lib)
    for name, count in KERNELS.items():
        hits = [v for k, v in meta.items() if name in k]
        assert len(hits) == count, (name, [k for k in meta if "track" in k])
        for v in hits:
            assert int(v["private_segment_fixed_size"]) == 0, v["name"]


# ----------------------------------------------------------------------------------------------- validation
def _status(fn):
    with pytest.raises(OrbxError) as e:
        fn()
    return e.value.status


def _host_only_matcher():
    return ORBmatcher(0.8, True, extractor=ORBextractor(1000, 1.2, 8, 20, 7, device=-2))


def _fake_batch(cap=512, nframes=2):
    """non-null 'device' addresses: a host-only handle never dereferences them (validation comes first, then ORBX_NO_DEVICE)"""
    return dict(nframes=nframes, keys_un=0x1000, desc=0x2000, u_right=None, counts=0x3000, cap=cap, cell_begin=0x4000,
                items=0x5000, bounds=tm.BOUNDS)


def test_host_only_validation(built_lib):
    m = _host_only_matcher()
    rng = np.random.default_rng(5)
    frame = tm.make_frame(rng, 50)
    fp = dict(tm.make_ff_problem(rng, frame, 40), frame=0)
    mp = dict(tm.make_mp_problem(rng, frame, 40, cap=512), frame=1)
    ff = lambda probs, batch=None: m.SearchByProjectionBatchDevice(probs, batch or _fake_batch(), K=tm.CAMERA, mb=tm.MB, mbf=tm.MBF,
                                                                   d_matched_last=0x6000, d_nmatches=0x7000)
    pp = lambda probs, batch=None: m.SearchByProjectionMapPointsBatchDevice(probs, batch or _fake_batch(), d_assigned=0x6000,
                                                                            d_nmatches=0x7000)
    # well-formed input reaches the device step
    assert _status(lambda: ff([fp, fp])) == _capi.NO_DEVICE
    assert _status(lambda: pp([mp, dict(mp, frame_observations=None)])) == _capi.NO_DEVICE
    # nothing to do
    assert ff([]) is None and pp([]) is None
    for call, good in ((ff, fp), (pp, dict(mp, frame_observations=None))):   # (the wrapper wants cap entries where there are any)
        assert _status(lambda: call([good, dict(good, frame=2)])) == _capi.BAD_ARGUMENT        # frame outside [0, nframes)
        assert _status(lambda: call([dict(good, frame=-1)])) == _capi.BAD_ARGUMENT
        assert _status(lambda: call([good], _fake_batch(cap=0))) == _capi.BAD_ARGUMENT
        assert _status(lambda: call([good], _fake_batch(cap=-3))) == _capi.BAD_ARGUMENT
        assert _status(lambda: call([good], _fake_batch(cap=65536))) == _capi.UNSUPPORTED
        assert _status(lambda: call([good], dict(_fake_batch(), counts=None))) == _capi.BAD_ARGUMENT
        assert _status(lambda: call([good], dict(_fake_batch(), bounds=(0, 0, 0, 150)))) == _capi.BAD_ARGUMENT
    # an octave / level outside [0, nlevels) counts only on a live point
    k_bad = fp["keys_un"].copy(); k_bad["octave"][3] = 8
    live, dead = fp["has_map_point"].copy(), fp["has_map_point"].copy()
    live[3], dead[3] = 1, 0
    assert _status(lambda: ff([fp, dict(fp, keys_un=k_bad, has_map_point=live)])) == _capi.BAD_ARGUMENT
    assert _status(lambda: ff([dict(fp, keys_un=k_bad, has_map_point=dead)])) == _capi.NO_DEVICE
    k_neg = fp["keys_un"].copy(); k_neg["octave"][3] = -1
    assert _status(lambda: ff([dict(fp, keys_un=k_neg, has_map_point=live)])) == _capi.BAD_ARGUMENT
    l_bad = mp["level"].copy(); l_bad[5] = 8
    view, away = mp["in_view"].copy(), mp["in_view"].copy()
    view[5], away[5] = 1, 0
    assert _status(lambda: pp([dict(mp, level=l_bad, in_view=view)])) == _capi.BAD_ARGUMENT
    assert _status(lambda: pp([dict(mp, level=l_bad, in_view=away)])) == _capi.NO_DEVICE


def test_host_only_raw_arguments(built_lib):
    """the raw C calls: nproblems < 0, null problem array, null fields of a non-empty view, empty views with null fields"""
    L = _capi.lib()
    m = _host_only_matcher()
    h = m._ex.handle
    rng = np.random.default_rng(6)
    frame = tm.make_frame(rng, 30)
    keep = []

    def frame_problem(p):
        P = _capi.TrackFrameProblem()
        P.frame, P.th, P.mono = 0, 15.0, 0
        a = [np.ascontiguousarray(p[k], t) for k, t in (("keys_un", _capi.KP_DTYPE), ("has_map_point", np.uint8),
                                                          ("world_pos", np.float32), ("mp_desc", np.uint8), ("observations", np.int32))]
        keep.extend(a)
        P.last.n = len(a[0])
        P.last.keys_un, P.last.has_map_point, P.last.world_pos, P.last.mp_desc, P.last.observations = (x.ctypes.data for x in a)
        return P

    def points_problem(p):
        P = _capi.TrackPointsProblem()
        P.frame, P.th = 0, 3.0
        a = [np.ascontiguousarray(p[k], t) for k, t in (("in_view", np.uint8), ("proj", np.float32), ("level", np.int32),
                                                          ("view_cos", np.float32), ("mp_desc", np.uint8), ("observations", np.int32))]
        keep.extend(a)
        P.points.n = len(a[0])
        (P.points.in_view, P.points.proj, P.points.level, P.points.view_cos, P.points.desc,
         P.points.observations) = (x.ctypes.data for x in a)
        return P

    bounds = np.asarray(tm.BOUNDS, np.float32); cam = np.asarray(tm.CAMERA, np.float32)
    dev = (2, 0x1000, 0x2000, None, 0x3000, 512, 0x4000, 0x5000)
    ff = lambda n, arr: L.orbx_search_by_projection_frame_batch_device(h, n, arr, *dev, _capi.ptr(cam), _capi.ptr(bounds), 0.1, 40.0,
                                                                       1, 0x6000, 0x7000)
    pp = lambda n, arr: L.orbx_search_by_projection_mappoints_batch_device(h, n, arr, *dev, _capi.ptr(bounds), 0.8, 0x6000, 0x7000)
    good_f, good_p = frame_problem(tm.make_ff_problem(rng, frame, 20)), points_problem(tm.make_mp_problem(rng, frame, 20))
    for fn, good, field in ((ff, good_f, ("last", "world_pos")), (pp, good_p, ("points", "proj"))):
        arr = (type(good) * 2)(good, good)
        assert fn(-1, arr) == _capi.BAD_ARGUMENT
        assert fn(2, None) == _capi.BAD_ARGUMENT
        assert fn(0, None) == _capi.OK
        assert fn(0, arr) == _capi.OK
        assert fn(2, arr) == _capi.NO_DEVICE
        setattr(getattr(arr[1], field[0]), field[1], None)          # a null field of a non-empty view
        assert fn(2, arr) == _capi.BAD_ARGUMENT
        getattr(arr[1], field[0]).n = 0                             # ... of an empty one: nothing is read
        assert fn(2, arr) == _capi.NO_DEVICE
        getattr(arr[1], field[0]).n = -1
        assert fn(2, arr) == _capi.BAD_ARGUMENT
    assert L.orbx_search_by_projection_frame_batch_device(None, 0, None, *dev, _capi.ptr(cam), _capi.ptr(bounds), 0.1, 40.0, 1,
                                                          0x6000, 0x7000) == _capi.BAD_ARGUMENT


# ----------------------------------------------------------------------------------------------- sanitizers
def test_packing_unit_clean_under_asan_ubsan(tmp_path):
    """csrc/orbx_track_pack.cpp (validation + packing, HIP-free) built with g++ -fsanitize=address,undefined together with
    tests/san_track_pack.cpp: 0 problems, empty views, n == cap, NULL frame_observations, every rejection of the table, and
    random problems whose packed block is read back in full"""
    exe = str(tmp_path / "san_track_pack")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_track_pack.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_track_pack.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr


# ----------------------------------------------------------------------------------------------- the planted edges hold what they claim
def test_planted_edges_do_what_they_are_planted_for():
    """the planted problems of tests/test_track_batch_gpu.py on the CPU: the oracle's result (both fp_modes) and the model's
    counters meet each case's expectation, and the model equals the oracle on them"""
    import test_track_batch_gpu as g
    scale = tm.scale_factors()
    cases = g.planted_ff_cases()
    assert len(cases) >= 20
    for name, fr, p, expect in cases:
        n, m, st = tm.model_ff(fr, p, True, scale)
        for fp in (oracle.FP_GCC_FMA, oracle.FP_STRICT):
            on, om = tm.oracle_ff(fr, p, True, fp, scale)
            assert expect(on, om, st), (name, on, st, om[:30])
            assert n == on and np.array_equal(m, om), name
    cases = g.planted_mp_cases()
    assert len(cases) >= 13
    for name, fr, p, expect in cases:
        po = p if p["frame_observations"] is not None else dict(p, frame_observations=np.full(g.CAP, -1, np.int32))
        on, oa = tm.oracle_mp(fr, po, 0.8, scale)
        n, a, st = tm.model_mp(fr, po, 0.8, scale)
        assert expect(on, oa, st), (name, on, st, oa[:30])
        assert n == on and np.array_equal(a, oa), name
