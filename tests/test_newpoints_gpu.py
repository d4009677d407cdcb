"""The per-match geometry of LocalMapping::CreateNewMapPoints on the device (orbx_create_new_map_points_batch: k_new_points) against
the library's host path (ORBX_NEWPOINTS=host on the same handle) and tests/newpoints_model.py, on the scenes of the CPU tests.
Every comparison is exact: status bytes, points as uint32.  Both fp_modes run the same scenes and must give the same bits.

Sizes: n in {1, 63, 64, 65, 129} (one lane, the chunk of 64 matches on both sides of its boundary, a last chunk with one live
lane); the full status scene list with every planted threshold pair; a mixed call of different n with two problems that launch
nothing, no problem at all, and each problem alone; the round driver on the device against the host-only handle's answer, with
the stand-in selection of the CPU tests and with the real one (orbx_triangulation_batch_select) against the loop of single calls.
At most 16 problems per call.  The model's answers are computed once per process (tests/newpoints_scenes.py)."""
import os

import numpy as np
import pytest

import newpoints_model as nm
import newpoints_scenes as sc
from orb_slam2_detailed_comments_amd import (ORBextractor, ORBmatcher, _capi, create_new_map_points_batch,
                                             create_new_map_points_rounds)
from orb_slam2_detailed_comments_amd.localmapping import matched_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[_capi.FP_GCC_FMA, _capi.FP_STRICT], ids=["fma", "strict"])
def ex(request):
    e = ORBextractor(1000, 1.2, 8, 20, 7, fp_mode=request.param)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def time_limit():
    """every test here is a GPU step with a limit of its own: a call that does not come back ends the process with a traceback"""
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def check(ex, problems, what):
    """device = model, then ORBX_NEWPOINTS=host on the same handle = model"""
    assert len(problems) <= 16
    out = None
    for env in (None, "host"):
        if env:
            os.environ["ORBX_NEWPOINTS"] = env
        try:
            res = create_new_map_points_batch(ex, problems)
        finally:
            os.environ.pop("ORBX_NEWPOINTS", None)
        sc.assert_equals_model(res, problems, f"{what}, ORBX_NEWPOINTS={env}")
        out = out or res
    return out


def test_size_list_device_equals_host_path_equals_model(ex):
    probs = list(sc.size_problems())
    assert tuple(len(p["matches"]) for p in probs) == sc.GPU_N
    check(ex, probs, "sizes")
    for p in probs:
        check(ex, [p], f"n = {len(p['matches'])} alone")


def test_every_case_of_the_scene_list(ex):
    sc.status_census()
    c = sc.cases()
    names = list(c)
    for i in range(0, len(names), 16):
        check(ex, [c[k] for k in names[i:i + 16]], f"cases {i}")


def test_mixed_call_with_problems_that_launch_nothing_and_no_problem_at_all(ex):
    mixed = sc.mixed_call()
    assert len(mixed) <= 16 and sum(len(p["matches"]) == 0 for p in mixed) == 2 and len({len(p["matches"]) for p in mixed}) >= 5
    inside = check(ex, mixed, "mixed")
    check(ex, [mixed[1], mixed[5]], "nothing launches")
    assert create_new_map_points_batch(ex, []) == []
    for k, p in enumerate(mixed):                                # a problem alone gives what it gives inside the batch
        (st, pts), = check(ex, [p], f"alone {k}")
        assert np.array_equal(st, inside[k][0]) and np.array_equal(pts.view(np.uint32), inside[k][1].view(np.uint32))


def same_points(a, b):
    return len(a) == len(b) and all(x[:3] == y[:3] and np.array_equal(x[3].view(np.uint32), y[3].view(np.uint32)) for x, y in zip(a, b))


def test_round_driver_on_the_device_equals_the_host_only_answer(ex):
    streams = sc.round_streams()
    host = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)         # (either fp_mode: the bits do not depend on it)
    try:
        want = create_new_map_points_rounds(host, streams)
    finally:
        host.close()
    got = create_new_map_points_rounds(ex, streams)
    assert all(same_points(g, w) and len(g) > 20 for g, w in zip(got, want))


def compute_f12(kf1, kf2):
    """LocalMapping::ComputeF12 in float64, rounded once: the caller's side of the interface"""
    R1, t1, R2, t2 = (np.asarray(kf1["Rcw"], np.float64), np.asarray(kf1["tcw"], np.float64), np.asarray(kf2["Rcw"], np.float64),
                      np.asarray(kf2["tcw"], np.float64))
    R12 = R1 @ R2.T
    t12 = -R1 @ R2.T @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    K = lambda kf: np.array([[kf["fx"], 0, kf["cx"]], [0, kf["fy"], kf["cy"]], [0, 0, 1]], np.float64)
    return (np.linalg.inv(K(kf1)).T @ tx @ R12 @ np.linalg.inv(K(kf2))).astype(np.float32)


def epipole(kf1, kf2):
    """the projection of KF1's centre into KF2, as SearchForTriangulation's caller gets it"""
    c = np.asarray(kf2["Rcw"], np.float64) @ np.asarray(kf1["Ow"], np.float64) + np.asarray(kf2["tcw"], np.float64)
    with np.errstate(all="ignore"):                              # a pure sideways motion puts it at infinity, as in the reference
        return float(kf2["fx"] * c[0] / c[2] + kf2["cx"]), float(kf2["fy"] * c[1] / c[2] + kf2["cy"])


def test_round_driver_with_the_real_selection_equals_the_loop_of_single_calls(ex):
    """the default selection (orbx_triangulation_batch_select) inside the driver against SearchForTriangulation, one call per
    neighbour, with the flags updated by hand: matching features carry the same random descriptor, all under one vocabulary node;
    one neighbour is gated"""
    rng = np.random.default_rng(3)
    streams = []
    for s in sc.round_streams(nstreams=2, nneigh=3):
        n1 = len(s["kf1"]["keys_un"])
        desc = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
        kf1 = dict(s["kf1"], desc=desc, feat_vec={0: list(range(n1))})
        nb = []
        for k, kf2 in enumerate(s["neighbours"]):
            if kf2 is None:
                nb.append(None)
                continue
            d2 = np.zeros((len(kf2["keys_un"]), 32), np.uint8)
            for a, b in s["cand"][k]:
                d2[b] = desc[a]
            nb.append(dict(kf2, desc=d2, feat_vec={0: list(range(len(d2)))}))
        streams.append(dict(kf1=kf1, neighbours=nb, F12=[None if k is None else compute_f12(kf1, k) for k in nb],
                            epipole=[None if k is None else epipole(kf1, k) for k in nb]))
    assert any(k is None for s in streams for k in s["neighbours"])
    got = create_new_map_points_rounds(ex, streams)
    m = ORBmatcher(0.6, False, extractor=ex)
    for s, g in zip(streams, got):
        has1 = s["kf1"]["has_map_point"].copy()
        want = []
        for k, kf2 in enumerate(s["neighbours"]):
            if kf2 is None:
                continue
            _, m12 = m.SearchForTriangulation(dict(s["kf1"], has_map_point=has1), kf2, s["F12"][k], s["epipole"][k])
            pairs = matched_pairs(m12)
            (st, pts), = create_new_map_points_batch(ex, [dict(kf1=s["kf1"], kf2=kf2, matches=pairs)])
            for (i1, i2), code, x in zip(pairs, st, pts):
                if code in nm.ACCEPTED:
                    has1[i1] = 1
                    want.append((k, int(i1), int(i2), x))
        assert same_points(g, want) and len(g) > 10 and {k for k, *_ in g} >= {0, 1}
