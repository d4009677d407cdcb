"""Tracking::SearchLocalPoints on the device (orbx_search_local_points_batch_device, orbx_predict_scale*), the part that needs no
GPU: the PredictScale threshold table against libm's own logf and against the compiled MapPoint.cc, the numpy model of the
frustum stage (tests/frustum_model.py) against hand-worked cases, the planted edges and the random scenes of
tests/test_local_points_gpu.py on the CPU, the ABI, validation before any device work on a host-only handle, the new kernel's
resources, and the HIP-free packing unit under AddressSanitizer + UndefinedBehaviorSanitizer (tests/san_local_pack.cpp, a
stand-alone program run as a child process)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frustum_model as fm
import track_model as tm
from orb_slam2_detailed_comments_amd import ORBextractor, ORBmatcher, OrbxError, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAMES = {"orbx_predict_scale_table": "orbx_status", "orbx_predict_scale": "int", "orbx_search_local_points_batch_device": "orbx_status"}


def _host_only_matcher(scale_factor=1.2, nlevels=8):
    return ORBmatcher(0.8, True, extractor=ORBextractor(1000, scale_factor, nlevels, 20, 7, device=-2))


# ----------------------------------------------------------------------------------------------- PredictScale
@pytest.mark.parametrize("scale_factor", [1.2, 2.0])
def test_table_equals_libm(built_lib, scale_factor):
    """the table is the model's (bisection with libm's logf through ctypes); orbx_predict_scale equals the reference's
    expression at every threshold and its two float neighbours on each side and at 10^6 seeded random ratios in [2^-4, 2^8]"""
    m = _host_only_matcher(scale_factor)
    thr = m.PredictScaleTable()
    want = fm.predict_scale_table(scale_factor, 8)
    assert np.array_equal(thr.view(np.int32), want.view(np.int32)), (thr, want)
    assert thr[0] == 0 and (np.diff(thr[1:]) > 0).all()
    for k in range(1, 8):
        for d in (-2, -1, 0, 1, 2):
            r = fm.step(thr[k], d)
            got, ref = m.PredictScale(r, 1.0), fm.clamped_scale(r, 1.0, scale_factor, 8)
            assert got == ref == (k if d >= 0 else k - 1), (k, d, r, got, ref)
    rng = np.random.default_rng(31)
    ratios = np.exp2(rng.uniform(-4.0, 8.0, 1_000_000)).astype(F32)
    L, h = _capi.lib(), m._ex.handle
    lsf = float(fm.logf(F32(scale_factor)))
    logf, predict = fm._libm.logf, L.orbx_predict_scale
    got = np.fromiter((predict(h, r, 1.0) for r in ratios.tolist()), np.int32, len(ratios))
    logs = np.fromiter((logf(r) for r in ratios.tolist()), F32, len(ratios))
    ref = np.clip(np.ceil(logs / F32(lsf)), 0, 7).astype(np.int32)         # one float division, ceilf, the clamp
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:10]
    assert len(set(got.tolist())) == 8
    # a division that is not by 1: the ratio is one correctly rounded float division
    a, b = rng.uniform(0.3, 30.0, 2000).astype(F32), rng.uniform(0.3, 30.0, 2000).astype(F32)
    for x, y in zip(a, b):
        assert m.PredictScale(x, y) == fm.clamped_scale(x, y, scale_factor, 8)


def test_predict_scale_outside_the_parity_contract(built_lib):
    """NaN and ratios <= 0 give 0, +inf gives nlevels - 1; nothing faults; no handle gives -1"""
    m = _host_only_matcher()
    inf, nan = float("inf"), float("nan")
    assert [m.PredictScale(a, b) for a, b in ((1.0, 0.0), (inf, 1.0), (nan, 1.0), (1.0, nan), (-1.0, 1.0), (0.0, 1.0), (0.0, 0.0), (-1.0, 0.0))] \
        == [7, 7, 0, 0, 0, 0, 0, 0]
    L = _capi.lib()
    assert L.orbx_predict_scale(None, 1.0, 1.0) == -1
    thr = np.zeros(8, F32)
    assert L.orbx_predict_scale_table(m._ex.handle, _capi.ptr(thr), 7) == _capi.BAD_ARGUMENT
    assert L.orbx_predict_scale_table(m._ex.handle, None, 8) == _capi.BAD_ARGUMENT
    assert L.orbx_predict_scale_table(None, _capi.ptr(thr), 8) == _capi.BAD_ARGUMENT
    # a scale factor whose levels outrun the finite floats: those thresholds are +inf and only an infinite ratio reaches them
    big = _host_only_matcher(scale_factor=1.0e10, nlevels=8)
    t = big.PredictScaleTable()
    assert np.isfinite(t[1:5]).all() and np.isinf(t[5:]).all(), t     # 1e10 .. 1e30 | 1e40 ..
    assert big.PredictScale(3.0e38, 1.0) == 4 and big.PredictScale(inf, 1.0) == 7


def test_table_equals_compiled_reference():
    """the compiled MapPoint::PredictScale (oracle/_ref/libref_matcher_*.so: h_predict_scale) at every threshold +- 1 ulp:
    dist = 1, so that mfMaxDistance / dist is the planted ratio itself, and a power of two beside it"""
    import ref_dbow2 as R
    from compat_scenes import F32 as CF32, KP, Harness, Scene, i32
    B = R.build_ref
    if B.reference_present():
        B.build()
    if not B.matcher_built():
        pytest.skip("neither oracle/_ref/libref_matcher_*.so nor the reference tree is here")
    thr = fm.predict_scale_table(1.2, 8)
    for variant in ("strict", "fma"):
        if variant == "fma" and not R.cpu_has_fma():
            continue
        H = Harness(B.matcher_lib_path(variant))
        S = Scene(H)
        f = S.frame(np.zeros(1, KP), np.zeros((1, 32), np.uint8))
        out = i32()
        for k in range(1, 8):
            for d, want in ((-1, k - 1), (0, k), (1, k)):
                for dist in (1.0, 4.0, 0.125):                        # ratio * 2^j / 2^j is the ratio again
                    dmax = F32(fm.step(thr[k], d) * F32(dist))
                    p = S.mp(np.zeros(32, np.uint8), dmin=float(dmax) / 8.0, dmax=float(dmax))
                    H("h_predict_scale", p, CF32(dist), f, 1, out)
                    assert int(out[0]) == want == fm.table_level(thr, F32(dmax / F32(dist))), (variant, k, d, dist, int(out[0]))


# ----------------------------------------------------------------------------------------------- the model
def test_model_on_hand_worked_cases():
    scale, thr = tm.scale_factors(), fm.predict_scale_table(1.2, 8)
    eye = np.eye(4, dtype=F32)
    pool = dict(world_pos=np.array([[0.25, 0.5, 2.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0]], F32),
                normal=np.array([[0, 0, 1], [0, 0, 0.25], [0, 0, 1], [0, 0, 1]], F32),
                min_distance=np.array([0.5, 0.5, 0.5, 2.0], F32), max_distance=np.array([4.0, 4.0, 4.0, 8.0], F32),
                mp_desc=np.zeros((4, 32), np.uint8), observations=np.ones(4, np.int32))
    prob = dict(th=F32(3.0), Tcw=eye, Ow=np.zeros(3, F32))
    for fma in (False, True):
        st = fm.frustum(prob, pool, scale, thr, fma)
        # point 0: Pc = P, invz = 0.5; u = 120 * 0.25 * 0.5 + 100 = 115, v = 118 * 0.5 * 0.5 + 75 = 104.5, ur = 115 - 40 * 0.5 = 95
        assert list(st["in_view"]) == [1, 0, 0, 0] and list(st["gate"]) == [0, 6, 1, 4]
        assert (st["proj_x"][0], st["proj_y"][0], st["proj_xr"][0]) == (115.0, 104.5, 95.0)
        dist = F32(np.sqrt(0.0625 + 0.25 + 4.0))                       # 2.0766...
        assert st["view_cos"][0] == F32(2.0 / np.float64(dist))
        # ratio 4 / 2.0766 = 1.926: between 1.2^3 = 1.728 and 1.2^4 = 2.0736 -> level 4; cos 0.963 <= 0.998: r = 4 * 3 * 1.2^4
        assert st["level"][0] == 4 and (st["min_level"][0], st["max_level"][0]) == (3, 4)
        assert st["r"][0] == F32(F32(F32(4.0) * F32(3.0)) * scale[4])
        assert st["r"][1] == -1 and st["min_level"][1] == -1
    # the camera centre moves the distance and the viewing angle, not the projection
    st = fm.frustum(dict(prob, Ow=np.array([0.0, 0.0, -2.0], F32), point_index=[1], viewing_cos_limit=0.25), pool, scale, thr, False)
    assert st["in_view"][0] == 1 and st["view_cos"][0] == 0.25 and st["proj_x"][0] == 100.0   # dist 3, ratio 4 / 3 -> level 2
    assert st["level"][0] == 2
    # th == 1 leaves the radius alone; a skipped point takes no part
    st = fm.frustum(dict(prob, th=F32(1.0), skip=[0, 1, 1, 1]), pool, scale, thr, True)
    assert st["r"][0] == F32(F32(4.0) * scale[4]) and list(st["gate"]) == [0, -1, -1, -1]


def test_planted_edges_do_what_they_are_planted_for():
    """the planted problems of tests/test_local_points_gpu.py on the CPU: in both fp_modes the model's gates, levels and the
    oracle's matches on the model's fields meet each case's expectation"""
    import test_local_points_gpu as g
    scale, thr = tm.scale_factors(), fm.predict_scale_table(1.2, 8)
    cases, frames, pool, probs = g.planted_call(thr)
    assert len(cases) >= 30
    for fma in (False, True):
        for (name, fr, _, _, expect), p in zip(cases, probs):
            st = fm.frustum(p, pool, scale, thr, fma)
            mp = fm.as_mp_problem(p, pool, st)
            mp["frame_observations"] = np.full(g.CAP, -1, np.int32)
            nm, row = tm.oracle_mp(fr, mp, g.NNRATIO, scale)
            assert expect(st["in_view"], st["level"], st["gate"], nm, row), (name, fma, st["in_view"], st["level"], st["gate"], nm, row[:8])


def test_random_scenes_are_honest():
    """every rejection gate fires, 20-80 % of the points are in view, >= 4 levels occur and the ordered pass rescans"""
    import test_local_points_gpu as g
    scale, thr = tm.scale_factors(), fm.predict_scale_table(1.2, 8)
    calls = g.random_scene()
    assert [len(c[2]) for c in calls] == [8, 3, 1] and [len(c[1]["world_pos"]) for c in calls] == [400, 257, 1]
    for fma in (False, True):
        g.assert_conditions(g.scene_conditions(calls, scale, thr, fma))


# ----------------------------------------------------------------------------------------------- ABI, code object
def test_symbols_declared_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "orbx.h")).read()
    L = _capi.lib()
    for name, ret in NAMES.items():
        assert f"{ret} {name}(" in header
        assert name in _capi.SYMBOLS
        assert hasattr(L, name)
    for t in ("orbx_local_map_view", "orbx_track_local_problem", "orbx_track_state"):
        assert f"}} {t};" in header
    assert L.orbx_abi_version() == 1
    assert C.sizeof(_capi.TrackLocalProblem) == 120 and C.sizeof(_capi.LocalMapView) == 56 and _capi.TRACK_STATE_DTYPE.itemsize == 20


def test_frustum_kernel_resources(built_lib):
    """k_track_frustum: one instance, no scratch, no LDS, blocks of 256, and the threshold table inside its argument segment"""
    from test_pipeline_room import _kernel_metadata
    meta = _kernel_metadata(built_lib)
    hits = [v for k, v in meta.items() if "k_track_frustum" in k]
    assert len(hits) == 1, [k for k in meta if "track" in k]
    v = hits[0]
    assert int(v["private_segment_fixed_size"]) == 0 and int(v["group_segment_fixed_size"]) == 0
    assert int(v["max_flat_workgroup_size"]) == 256
    assert int(v["kernarg_segment_size"]) >= 10 * 4 + 4 + 2 * 16 * 4 + 9 * 8
    # the three kernels behind it are the ones the map-point call runs
    for name, count in {"k_track_project": 1, "k_track_cand": 2, "k_track_select": 2}.items():
        assert len([k for k in meta if name in k]) == count


# ----------------------------------------------------------------------------------------------- validation
def _fails(fn, status, text):
    with pytest.raises(OrbxError) as e:
        fn()
    assert e.value.status == status and text in str(e.value), (e.value.status, str(e.value))


def _fake_batch(cap=512, nframes=2):
    return dict(nframes=nframes, keys_un=0x1000, desc=0x2000, u_right=None, counts=0x3000, cap=cap, cell_begin=0x4000,
                items=0x5000, bounds=tm.BOUNDS)


def test_host_only_validation(built_lib):
    m = _host_only_matcher()
    rng = np.random.default_rng(5)
    frame = tm.make_frame(rng, 50)
    T = tm._pose(rng)
    pool = fm.make_pool(rng, frame, 40, T)
    good = fm.make_problem(rng, 1, T, 40, 512)
    call = lambda probs, lm=pool, batch=None, **kw: m.SearchLocalPointsBatchDevice(
        probs, lm, batch or _fake_batch(), K=tm.CAMERA, mbf=tm.MBF, **dict(dict(d_assigned=0x6000, d_nmatches=0x7000), **kw))
    # well-formed input reaches the device step; the optional outputs and fields may be absent
    _fails(lambda: call([good, good]), _capi.NO_DEVICE, "no device handle")
    _fails(lambda: call([dict(good, point_index=None, skip=None, frame_observations=None)], d_in_view=0x8000, d_track=0x9000),
           _capi.NO_DEVICE, "no device handle")
    assert call([]) is None and call([], None) is None
    _fails(lambda: call([good, dict(good, frame=2)]), _capi.BAD_ARGUMENT, "frame outside")
    _fails(lambda: call([dict(good, frame=-1)]), _capi.BAD_ARGUMENT, "frame outside")
    _fails(lambda: call([good], batch=_fake_batch(cap=0)), _capi.BAD_ARGUMENT, "cap <= 0")
    _fails(lambda: call([good], batch=_fake_batch(cap=-3)), _capi.BAD_ARGUMENT, "cap <= 0")
    _fails(lambda: call([dict(good, frame_observations=None)], batch=_fake_batch(cap=65536)), _capi.UNSUPPORTED, "cap > 65535")
    _fails(lambda: call([good], batch=dict(_fake_batch(), counts=None)), _capi.BAD_ARGUMENT, "null device buffer")
    _fails(lambda: call([good], d_assigned=None), _capi.BAD_ARGUMENT, "null device buffer")
    _fails(lambda: call([good], batch=dict(_fake_batch(), bounds=(0, 0, 0, 150))), _capi.BAD_ARGUMENT, "bad image bounds")
    for bad in (40, -1, 2 ** 31 - 1):
        idx = good["point_index"].copy(); idx[-1] = bad
        _fails(lambda: call([good, dict(good, point_index=idx)]), _capi.BAD_ARGUMENT, "point_index outside the pool")
    _fails(lambda: call([good], None), _capi.BAD_ARGUMENT, "null local map")
    _fails(lambda: call([good], dict(pool, **{k: pool[k][:0] for k in pool})), _capi.BAD_ARGUMENT, "point_index outside the pool")


def test_host_only_raw_arguments(built_lib):
    """the raw C call: nproblems < 0, a null problem array, each null field of a non-empty pool, an empty pool with null fields,
    npoints < 0, a NULL point_index whose npoints is not the pool's"""
    L = _capi.lib()
    m = _host_only_matcher()
    h = m._ex.handle
    M = 20
    arrays = dict(world_pos=np.zeros((M, 3), F32), normal=np.zeros((M, 3), F32), min_distance=np.ones(M, F32),
                  max_distance=np.ones(M, F32), desc=np.zeros((M, 32), np.uint8), observations=np.zeros(M, np.int32))
    mv = _capi.LocalMapView()
    mv.n = M
    for k, a in arrays.items():
        setattr(mv, k, a.ctypes.data)
    idx = np.arange(M, dtype=np.int32)
    P = _capi.TrackLocalProblem()
    P.frame, P.th, P.viewing_cos_limit, P.npoints, P.point_index = 0, 3.0, 0.5, M, idx.ctypes.data
    arr = (_capi.TrackLocalProblem * 2)(P, P)
    bounds = np.asarray(tm.BOUNDS, F32); cam = np.asarray(tm.CAMERA, F32)
    dev = (2, 0x1000, 0x2000, None, 0x3000, 512, 0x4000, 0x5000)
    fn = lambda n, a, lm: L.orbx_search_local_points_batch_device(h, n, a, lm, *dev, _capi.ptr(cam), _capi.ptr(bounds), 40.0, 0.8,
                                                                  0x6000, 0x7000, None, None)
    why = lambda: L.orbx_last_error().decode()
    assert fn(-1, arr, C.byref(mv)) == _capi.BAD_ARGUMENT and "nproblems < 0" in why()
    assert fn(2, None, C.byref(mv)) == _capi.BAD_ARGUMENT and "null problem array" in why()
    assert fn(0, None, None) == _capi.OK and fn(0, arr, C.byref(mv)) == _capi.OK
    assert fn(2, arr, C.byref(mv)) == _capi.NO_DEVICE
    for k in arrays:
        keep = getattr(mv, k)
        setattr(mv, k, None)
        assert fn(2, arr, C.byref(mv)) == _capi.BAD_ARGUMENT and "null field of a local-map view" in why(), k
        setattr(mv, k, keep)
    arr[1].npoints = -1
    assert fn(2, arr, C.byref(mv)) == _capi.BAD_ARGUMENT and "npoints < 0" in why()
    arr[1].npoints, arr[1].point_index = M - 1, None
    assert fn(2, arr, C.byref(mv)) == _capi.BAD_ARGUMENT and "point_index is NULL" in why()
    arr[1].npoints = M                                             # the whole pool in order
    assert fn(2, arr, C.byref(mv)) == _capi.NO_DEVICE
    mv.n = -1
    assert fn(2, arr, C.byref(mv)) == _capi.BAD_ARGUMENT and "map.n < 0" in why()
    empty = _capi.LocalMapView()                                    # an empty pool: nothing of it is read
    arr[0].npoints = arr[1].npoints = 0
    assert fn(2, arr, C.byref(empty)) == _capi.NO_DEVICE and fn(2, arr, None) == _capi.NO_DEVICE
    assert L.orbx_search_local_points_batch_device(None, 0, None, None, *dev, _capi.ptr(cam), _capi.ptr(bounds), 40.0, 0.8, 0x6000,
                                                   0x7000, None, None) == _capi.BAD_ARGUMENT


# ----------------------------------------------------------------------------------------------- sanitizers
def test_packing_unit_clean_under_asan_ubsan(tmp_path):
    """csrc/orbx_track_pack.cpp (validation, packing, the PredictScale table; HIP-free) built with g++
    -fsanitize=address,undefined together with tests/san_local_pack.cpp and run as a child process: the table against the
    expression it inverts, every rejection, empty pools and problems, NULL optional fields, and random calls whose packed
    block is read back in full"""
    exe = str(tmp_path / "san_local_pack")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_local_pack.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_track_pack.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr
