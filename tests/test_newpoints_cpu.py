"""The per-match geometry of LocalMapping::CreateNewMapPoints (orbx_create_new_map_points_batch) and the round driver
(create_new_map_points_rounds), the part that needs no GPU: the library's host path through the C ABI against
tests/newpoints_model.py, bit for bit -- status bytes, points as uint32 -- in both fp_modes; the planted edges ON THE MODEL ALONE;
validation before any work; empty calls; a problem alone against the same problem inside a batch; the round driver against the
sequential loop; the distance of cos(2 * atan2(mb / 2, depth)) from the C library's cosf / atan2f; the HIP-free unit under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/san_newpoints.cpp, a stand-alone program); no scratch and no LDS in
k_new_points.

The contract is device = host path = model.  Parity with an OpenCV build is not pinned."""
import ctypes as C
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

import newpoints_model as nm
import newpoints_scenes as sc
from orb_slam2_detailed_comments_amd import ORBextractor, _capi, create_new_map_points_batch, create_new_map_points_rounds
from orb_slam2_detailed_comments_amd.localmapping import _keyframe, matched_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
# largest |orbx_newpoints_stereo_cos - cosf(2 * atan2f(mb / 2, depth))| over depth / mb in [1, 1e4], measured on the CPU and
# recorded in DESIGN.md F17: one ulp of a float just below 1
STEREO_COS_MEASURED = 5.960e-8


@pytest.fixture(scope="module", params=[_capi.FP_GCC_FMA, _capi.FP_STRICT], ids=["fma", "strict"])
def host(request, built_lib):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2, fp_mode=request.param)
    yield ex
    ex.close()


def run(host, problems, what=""):
    res = create_new_map_points_batch(host, problems)
    sc.assert_equals_model(res, problems, what)
    return res


def test_the_model_alone_reaches_every_status_but_two_and_shows_the_planted_edges(built_lib):
    seen = sc.status_census()
    assert nm.ZERO_W not in seen and nm.ZERO_DIST not in seen and len(seen) == 10
    c = sc.cases()
    for name in c:                                               # each planted pair straddles its threshold
        if name.endswith("_under"):
            under, over = sc.model_of(c[name])[0][0], sc.model_of(c[name[:-6] + "_over"])[0][0]
            assert under in nm.ACCEPTED and over not in nm.ACCEPTED, name


def test_every_case_equals_the_model(host):
    c = sc.cases()
    res = dict(zip(c, run(host, list(c.values()), "cases")))
    st, pts = res["stereo_paths"]
    assert st[1] == nm.STEREO1 and st[2] == nm.STEREO2 and pts[1].any() and not pts[0].any() and not pts[5].any()
    assert np.isin(res["general"][0], nm.ACCEPTED).sum() > 100


def test_size_list_mixed_call_empty_calls_and_single_calls(host):
    run(host, list(sc.size_problems()), "sizes")
    mixed = sc.mixed_call()
    assert len(mixed) <= 16 and sum(len(p["matches"]) == 0 for p in mixed) == 2
    inside = run(host, mixed, "mixed")
    for k, p in enumerate(mixed):                                # a problem alone gives what it gives inside the batch
        (st, pts), = run(host, [p], f"alone {k}")
        assert np.array_equal(st, inside[k][0]) and np.array_equal(pts.view(np.uint32), inside[k][1].view(np.uint32))
    assert create_new_map_points_batch(host, []) == []
    (st, pts), (st2, pts2) = create_new_map_points_batch(host, [mixed[1], mixed[5]])
    assert st.shape == (0,) and pts.shape == (0, 3) and st2.shape == (0,) and pts2.shape == (0, 3)


def test_validation_before_any_work(host):
    L, B, OK = _capi.lib(), _capi.BAD_ARGUMENT, _capi.OK
    p = sc.cases()["general"]
    n = len(p["matches"])
    arr = (_capi.NewPointsProblem * 2)()
    keep = []
    m = p["matches"].copy()
    status, points = np.zeros(2 * n, np.uint8), np.zeros((2 * n, 3), F)

    def fill():
        for a in arr:
            _keyframe(p["kf1"], a.kf1, keep)
            _keyframe(p["kf2"], a.kf2, keep)
            a.scale_factor, a.nmatches, a.matches = 1.2, n, m.ctypes.data

    def call(nprob=2, pr=arr, h=host.handle, st=status, pt=points):
        return L.orbx_create_new_map_points_batch(h, nprob, C.cast(pr, C.c_void_p) if pr is not None else None, _capi.ptr(st),
                                                  _capi.ptr(pt))

    fill()
    assert call() == OK
    assert call(nprob=-1) == B and call(pr=None) == B and call(h=None) == B and call(st=None) == B and call(pt=None) == B
    assert call(nprob=0, pr=None, st=None, pt=None) == OK
    fill()
    arr[1].nmatches = -1
    assert call() == B
    fill()
    arr[1].matches = None
    assert call() == B
    for kf in ("kf1", "kf2"):
        for field in ("keys_un", "keys", "u_right", "depth", "scale_factors", "level_sigma2"):
            fill()
            setattr(getattr(arr[1], kf), field, None)
            assert call() == B, (kf, field)
        for field in ("n", "nlevels"):
            fill()
            setattr(getattr(arr[1], kf), field, -1)
            assert call() == B, (kf, field)
    for col, bad in ((0, len(p["kf1"]["keys_un"])), (0, -1), (1, len(p["kf2"]["keys_un"])), (1, -1)):   # an index outside its keyframe
        fill()
        m[5, col] = bad
        assert call() == B, (col, bad)
        m[:] = p["matches"]
    assert b"index" in L.orbx_last_error()
    for kf, col in (("kf1", 0), ("kf2", 1)):                    # an octave outside the scale tables
        for bad in (-1, 8):
            q = dict(p, **{kf: dict(p[kf], keys_un=p[kf]["keys_un"].copy())})
            q[kf]["keys_un"]["octave"][m[7, col]] = bad
            with pytest.raises(_capi.OrbxError) as e:
                create_new_map_points_batch(host, [p, q])
            assert e.value.status == B and "octave" in str(e.value)
        fill()
        getattr(arr[1], kf).nlevels = int(p[kf]["keys_un"]["octave"][m[:, col]].max())   # the table ends below a matched feature's octave
        assert call() == B
    fill()                                                       # a problem without a match reads none of its arrays
    arr[1].nmatches, arr[1].matches = 0, None
    for kf in (arr[1].kf1, arr[1].kf2):
        kf.keys_un = kf.keys = kf.u_right = kf.depth = kf.scale_factors = kf.level_sigma2 = None
    assert call() == OK
    arr[0].nmatches = 0
    assert call(st=None, pt=None) == OK                          # nothing to write: the outputs may be null


def sequential(host, stream):
    """the loop of :378-679 for one stream: neighbour by neighbour through single-problem calls, the flags updated by hand"""
    has1 = stream["kf1"]["has_map_point"].copy()
    out = []
    for k, kf2 in enumerate(stream["neighbours"]):
        if kf2 is None:
            continue
        has2 = kf2["has_map_point"].copy()
        pairs = matched_pairs(stream["select"](k, has1.copy(), has2.copy()))
        (st, pts), = create_new_map_points_batch(host, [dict(kf1=stream["kf1"], kf2=kf2, matches=pairs)])
        for (i1, i2), s, x in zip(pairs, st, pts):
            if s in nm.ACCEPTED:
                has1[i1] = 1
                out.append((k, int(i1), int(i2), x))
    return out


def same_points(a, b):
    return len(a) == len(b) and all(x[:3] == y[:3] and np.array_equal(x[3].view(np.uint32), y[3].view(np.uint32)) for x, y in zip(a, b))


def test_rounds_for_three_streams_equal_each_stream_alone_neighbour_by_neighbour(host):
    streams = sc.round_streams()
    assert len(streams) == 3 and all(len(s["neighbours"]) == 4 for s in streams) and streams[1]["neighbours"][2] is None
    flags = [s["kf1"]["has_map_point"].copy() for s in streams]
    got = create_new_map_points_rounds(host, streams)
    assert all(np.array_equal(f, s["kf1"]["has_map_point"]) for f, s in zip(flags, streams))   # the caller's flags are not modified
    again = 0
    for s, g in zip(streams, got):
        want = sequential(host, s)
        assert same_points(g, want) and len(g) > 20
        assert [k for k, *_ in g] == sorted(k for k, *_ in g) and len({i1 for _, i1, *_ in g}) == len(g)   # creation order, once each
        assert not any(s["kf1"]["has_map_point"][i1] for _, i1, *_ in g)
        assert {k for k, *_ in g} >= {0, 1}                     # later neighbours still create points: from what earlier ones rejected
        for k, i1, i2, _ in g:                                   # accepted for k; the selection of a later neighbour, run with the
            for later in range(k + 1, len(s["neighbours"])):     # flags from before the loop, would have matched it again
                kf2 = s["neighbours"][later]
                if kf2 is not None and s["select"](later, s["kf1"]["has_map_point"], kf2["has_map_point"])[i1] >= 0:
                    again += 1
                    break
    assert again > 20
    alone = [create_new_map_points_rounds(host, [s])[0] for s in streams]
    assert all(same_points(a, g) for a, g in zip(alone, got))
    assert create_new_map_points_rounds(host, []) == []


def test_distance_of_the_stereo_cosine_from_the_c_library(built_lib):
    """cos(2 * atan2(mb / 2, depth)) in float, as the reference's overloads resolve, by the C library against the library's own, over
    depth / mb in [1, 1e4]: 200001 ratios, log-spaced, at two baselines.  The test asserts twice the recorded figure: the margin
    only absorbs another libm."""
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.atan2f.restype = libm.cosf.restype = C.c_float
    libm.atan2f.argtypes = [C.c_float, C.c_float]
    libm.cosf.argtypes = [C.c_float]
    L = _capi.lib()
    worst = 0.0
    for mb in (F(0.1), F(0.537)):
        for r in np.logspace(0, 4, 100001):
            d = F(mb * F(r))
            ref = libm.cosf(F(2) * F(libm.atan2f(mb / F(2), d)))
            worst = max(worst, abs(float(L.orbx_newpoints_stereo_cos(mb, d)) - float(ref)))
    print(f"stereo cosine: largest distance from libm {worst:.3e}")
    assert worst <= 2 * STEREO_COS_MEASURED


def test_host_unit_clean_under_asan_ubsan(tmp_path):
    """csrc/orbx_newpoints.cpp (validation, packing, the host path, the scatter; HIP-free) built with
    g++ -fsanitize=address,undefined together with tests/san_newpoints.cpp, a stand-alone program: sizes around the chunk of 64,
    every stereo combination, problems without a match, non-finite input, every validation failure"""
    exe = str(tmp_path / "san_newpoints")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_newpoints.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_newpoints.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr


def test_kernel_has_no_scratch_and_no_lds(built_lib):
    from test_pipeline_room import _kernel_metadata
    hits = [v for k, v in _kernel_metadata(built_lib).items() if "k_new_points" in k]
    assert len(hits) == 1
    assert int(hits[0]["private_segment_fixed_size"]) == 0 and int(hits[0]["group_segment_fixed_size"]) == 0
    assert int(hits[0]["vgpr_count"]) <= 128                     # 58 when this was written; 128 keeps four waves per SIMD
