"""Optimizer::PoseOptimization(Frame*) (orbx_pose_optimization, orbx_pose_optimization_batch_device), the part that needs no GPU:
the library's host path through the C ABI against tests/pose_model.py, bit for bit on the pose floats, the outlier bytes and
the inlier count; synthetic scenes with a known pose; every branch of the Levenberg-Marquardt control asserted from the
model's trace on committed seeds; the size list; validation before any work; the HIP-free unit under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/san_pose_pack.cpp, a stand-alone program); no scratch in k_pose_opt.

The contract is the one of tests/frustum_model.py: device = host path = model.  Parity with a g2o + Eigen build is not pinned
(DESIGN.md section 2, F11).

Stale errors.  After a rejected trial the edges keep that trial's errors and the inlier test reads them (pose_model.py and the
library both evaluate the non-outlier edges at the pose where computeActiveErrors ran last).  The rule is pinned by
test_inlier_test_reads_stale_errors_for_inliers_and_fresh_ones_for_outliers: orbx_debug_pose_inlier_test runs the library's
inlier test with the two poses given a few centimetres apart, and the scene gives other flags under either one-pose rule.
Inside a whole optimisation the rule is reached (`last_rejected` and `last_differs` in the trace of the committed seeds and of
the ray scene, library = model bit for bit) but changes no flag there, and no scene was found in which it does: a rejected LAST
trial needs ten rejections in a row (lambda grown by 2^45), rho == 0 or a NaN rho, so with finite terms its pose differs from
the restored one by about 1e-16.  A flag then flips only for an edge with chi2 at the threshold whose gradient is about 1e9,
which makes its Hessian part about 1e13 times the rest (gradient^2 = 24 x Hessian part at chi2 = 6); such an edge has to be held
in balance by a twin, the pair's constant chi2 of 12 then triggers the "Raul" stop, whose last trial is accepted.  600 random
seeds and 1 440 constructed stiff-pair scenes (point 1e-3 to 1e-5 m from the camera centre, invSigma2 1e6 to 1e10) gave
`stale_flips` == 0 everywhere."""
import os
import re
import subprocess

import numpy as np
import pytest

import pose_model as pm
import pose_scenes as ps
from pose_cases import (BRANCH_SEEDS, CAP, SIZES, assert_inlier_test, assert_rows, assert_same, bits, branch_scenes, model, run_batch, single,  # noqa: F401
                        run_inlier_test, size_scenes, special_scenes, stale_case)
from orb_slam2_detailed_comments_amd import ORBextractor, OrbxError, _capi, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(built_lib):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    yield ex
    ex.close()


# ----------------------------------------------------------------------------------------------- scenes with a known pose
@pytest.mark.parametrize("mode", ["mono", "stereo", "mixed"])
def test_noise_free_observations_give_the_true_pose(host, mode):
    s = ps.make(1, 60, mode)
    assert np.abs(s["Tcw0"] - s["Tcw_true"]).max() > 5e-3          # the start is a few centimetres / a degree off
    want = model(s)
    got = single(host, s)
    assert_same(got, want, mode)
    assert np.abs(got[0] - s["Tcw_true"]).max() < 1e-5
    assert got[2] == 60 and not got[1].any()


@pytest.mark.parametrize("mode", ["mono", "stereo", "mixed"])
def test_noise_and_planted_outliers(host, mode):
    s = ps.make(2, 150, mode, noise=1.0, outlier_frac=0.2)
    want = model(s)
    got = single(host, s)
    assert_same(got, want, mode)
    planted = s["planted"] & (s["gross"] > 10)
    assert planted.sum() >= 15 and got[1][planted].all()            # every planted outlier beyond 10 sigma is flagged
    assert got[2] == want[2] and got[2] >= 100
    assert (got[1][s["point"] < 0] == 0).all()


# ----------------------------------------------------------------------------------------------- branches, from the trace
def test_every_branch_of_the_lm_control_is_reached_and_agrees(host):
    scenes, models, traces = branch_scenes()
    rounds = [r for t in traces for r in t["rounds"]]
    iters = [i for r in rounds for i in r["iters"]]
    trials = [t for i in iters for t in i["trials"]]
    assert any(not t["accepted"] for t in trials)                               # a rejected trial (pose restored)
    assert any(t["nu"] > 2 for t in trials)                                     # nu doubled: a second rejection in a row
    assert any(i["end"] == "trials" and len(i["trials"]) == 10 for i in iters)  # the 10-trial Terminate
    assert any(i["end"] == "stall" for i in iters)                              # the "Raul" stop
    assert any(r["reentered"] > 0 for r in rounds)                              # an outlier passes again in a later round
    assert any(r["round"] == 3 and r.get("nonunit_huber", 0) > 0 for r in rounds)   # round 4 is not what Huber would give
    assert any(t.get("theta_small", 0) > 0 for t in traces)                     # the theta < 1e-5 branch of exp
    assert any(r["last_rejected"] and r["last_differs"] for r in rounds)        # stale errors of a rejected last trial are read
    assert all(np.isfinite(t["chi"]) for t in trials if t["accepted"])
    for s, want, (seed, n, mode) in zip(scenes, models, BRANCH_SEEDS):
        assert_same(single(host, s), want, f"seed {seed}")


def test_round_four_runs_without_huber(host):
    """the same scene with the kernel kept on in round 4 ends elsewhere: the library follows the model that takes it off"""
    scenes, models, traces = branch_scenes()
    import unittest.mock as mock
    differs = 0
    for s, want in zip(scenes, models):
        orig = pm._huber
        with mock.patch.object(pm, "_huber", lambda chi2, stereo, robust: orig(chi2, stereo, True)):
            kept = model(s)
        differs += not np.array_equal(bits(kept[0]), bits(want[0]))
    assert differs >= 1


def test_special_scenes_are_defined_by_the_model(host):
    seen = {}
    for name, s, kw in special_scenes():
        tr = {}
        want = model(s, trace=tr, **kw)
        got = single(host, s, **kw)
        assert_same(got, want, name)
        assert np.isfinite(got[0]).all(), name
        seen[name] = tr["rounds"]
    assert any(r["nactive"] == 0 and not r["iters"] for r in seen["all-gross"][1:])      # a round with no active edge
    assert single(host, special_scenes()[0][1])[2] == 0
    fails = [t["ok"] for r in seen["zero-information"] for i in r["iters"] for t in i["trials"]]
    assert fails and not any(fails)                                                        # every solve fails, 10 trials, Terminate
    assert all(r["iters"][-1]["end"] == "trials" for r in seen["zero-information"])
    # all points on one ray: lambda > 0 keeps every pivot of the unpivoted L D L^T positive, so the solve does NOT fail here;
    # the rank-deficient system ends through rho == 0 (mono) with a rejected last trial
    assert any(r["iters"][-1]["end"] == "rho0" and r["last_rejected"] for r in seen["ray-mono"])


def test_inlier_test_reads_stale_errors_for_inliers_and_fresh_ones_for_outliers(host):
    """The rule itself, where it shows: orbx_debug_pose_inlier_test runs the inlier test of the host path with the estimate and
    the pose of the last trial given, a few centimetres apart.  An edge flagged outlier is tested at the estimate, every other
    edge at the last trial's pose; testing all edges at either pose gives other flags (asserted)."""
    s, est, last, flags, want = stale_case()
    assert_inlier_test(run_inlier_test(host, s, est, last, flags), s, est, last, flags, want)


def test_point_at_z_zero_ends_and_nothing_is_accepted(host):
    """Outside the contract: one point sits exactly at z = 0 of the START pose's camera frame, so every chi2 sum is NaN and
    every rho is NaN; each iteration of the first round makes one rejected trial, ten iterations run, and the pose stays the start
    pose (which is far from the scene's, so the later rounds have no active edge)."""
    s = ps.make(3, 40, "mono", noise=1.0, outlier_frac=0.2)
    T0 = np.eye(4, dtype=np.float32)
    T0[:3, 3] = (0.25, -0.125, 0.5)
    world = s["world"].copy()
    first = s["point"][s["point"] >= 0][0]
    world[first] = (1.0, 2.0, -0.5)                                   # z = -0.5 + 0.5 = 0 exactly
    s = ps.variant(s, Tcw0=T0, world=world)
    tr = {}
    want = model(s, trace=tr)
    trials = [t for r in tr["rounds"] for i in r["iters"] for t in i["trials"]]
    assert trials and not any(t["accepted"] for t in trials)          # nothing non-finite is accepted
    r0 = tr["rounds"][0]
    assert len(r0["iters"]) == 10 and all(len(i["trials"]) == 1 for i in r0["iters"]) and r0["last_rejected"]
    got = single(host, s)
    assert_same(got, want, "z = 0")
    assert np.array_equal(bits(got[0]), bits(pm.to_cvmat(pm.to_se3quat(T0))))     # the pose is the start pose, converted


@pytest.mark.parametrize("poison", [(np.inf, 1.0, 2.0), (np.nan, np.nan, np.nan), (1e30, -1e30, 1e-30), (0.0, 0.0, 0.0)])
def test_non_finite_input_ends_and_is_never_accepted(host, poison):
    s = ps.make(4, 30, "mixed", noise=1.0)
    world = s["world"].copy()
    world[s["point"][s["point"] >= 0][:3]] = poison
    s = ps.variant(s, world=world)
    tr = {}
    want = model(s, trace=tr)
    assert all(np.isfinite(t["chi"]) for r in tr["rounds"] for i in r["iters"] for t in i["trials"] if t["accepted"])
    assert_same(single(host, s), want, str(poison))


def test_point_behind_the_camera_is_inside_the_contract(host):
    s = ps.make(5, 40, "mixed", noise=1.0)
    world = s["world"].copy()
    T = s["Tcw_true"].astype(np.float64)
    behind = np.array([0.3, -0.2, -4.0])                              # camera frame, z < 0, finite terms
    world[s["point"][s["point"] >= 0][:2]] = ((behind - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    s = ps.variant(s, world=world)
    want = model(s)
    got = single(host, s)
    assert_same(got, want, "behind")
    assert np.isfinite(got[0]).all() and got[2] >= 30


# ----------------------------------------------------------------------------------------------- sizes, batches
@pytest.mark.parametrize("use_index", [True, False], ids=["index", "pool-order"])
def test_size_list_as_one_batch(host, use_index):
    scenes, models = size_scenes()
    want = ps.expected(scenes, CAP, models)
    assert_rows(run_batch(host, scenes, use_index=use_index), want, "sizes")
    T, o, n = want
    assert (T[:2] == ps.PREFILL_T).all() and (n[:2] == 0).all()       # 0 and 2 edges: the pose row stays, 0 inliers
    assert (T[2:] != ps.PREFILL_T).any(axis=1).all()
    assert (o[:, :].ravel() == ps.PREFILL_OUTLIER).any()              # entries without a MapPoint are not written


def test_break_after_round_one_below_ten_edges(host):
    tr9, tr10 = {}, {}
    scenes, _ = size_scenes()
    model(scenes[SIZES.index(9)], trace=tr9)
    model(scenes[SIZES.index(10)], trace=tr10)
    assert len(tr9["rounds"]) == 1 and len(tr10["rounds"]) == 4


def test_shared_frame_and_batch_equals_single_calls(host):
    s = ps.make(6, 80, "mixed", noise=1.0, outlier_frac=0.1)
    s2 = ps.variant(s, Tcw0=ps.make(7, 80, "mixed")["Tcw0"] @ np.linalg.inv(ps.make(7, 80, "mixed")["Tcw_true"]) @ s["Tcw_true"])
    s2["Tcw0"] = s2["Tcw0"].astype(np.float32)
    s3 = ps.make(8, 30, "stereo", noise=1.0)
    scenes = [s, s2, s3]
    models = [model(x) for x in scenes]
    want = ps.expected(scenes, CAP, models)
    # s3's frame is shorter than s's; problems 0 and 1 name frame 0
    assert_rows(run_batch(host, scenes, frame_of=[0, 0, 1]), want, "shared frame")
    for k, x in enumerate(scenes):                                    # one problem per call
        one = run_batch(host, [x])
        assert_rows(one, [w[k:k + 1] for w in want], f"single {k}")
        assert_same(single(host, x), models[k], f"single-call form {k}")


# ----------------------------------------------------------------------------------------------- validation
def _status(fn):
    with pytest.raises(OrbxError) as e:
        fn()
    return e.value.status


def test_validation_before_any_work(host):
    L, h, P = _capi.lib(), host.handle, _capi.ptr
    B, U, OK = _capi.BAD_ARGUMENT, _capi.UNSUPPORTED, _capi.OK
    s = ps.make(9, 12, "mixed", nfeat=16)
    b = ps.batch([s, s], 16, frame_of=[0, 0])
    prob = (_capi.PoseProblem * 2)()
    idx = [np.ascontiguousarray(p["point_index"], np.int32) for p in b["problems"]]
    for k in range(2):
        prob[k].frame = 0
        prob[k].Tcw[:] = s["Tcw0"].reshape(16).tolist()
        prob[k].point_index = idx[k].ctypes.data
        prob[k].npoints = len(idx[k])
    T = np.full((2, 16), ps.PREFILL_T, np.float32)
    o = np.full((2, 16), ps.PREFILL_OUTLIER, np.uint8)
    n = np.full(2, ps.PREFILL_N, np.int32)
    keys = b["keys"].copy()
    args = dict(np_=2, pr=prob, npool=len(b["world"]), w=b["world"], nf=1, k=keys, ur=b["u_right"], c=b["counts"], cap=16, pt=b["point"],
                cam=ps.CAMERA4, sig=ps.INV_SIGMA2, nl=8, T=T, o=o, n=n)

    def call(**kw):
        a = dict(args)
        a.update(kw)
        import ctypes as C
        st = L.orbx_pose_optimization_batch_device(h, a["np_"], C.cast(a["pr"], C.c_void_p) if a["pr"] is not None else None, a["npool"],
                                                   P(a["w"]), a["nf"], P(a["k"]), P(a["ur"]), P(a["c"]), a["cap"], P(a["pt"]), P(a["cam"]),
                                                   float(ps.MBF), P(a["sig"]), a["nl"], P(a["T"]), P(a["o"]), P(a["n"]))
        if st != OK:     # nothing is written on failure
            assert (T == ps.PREFILL_T).all() and (o == ps.PREFILL_OUTLIER).all() and (n == ps.PREFILL_N).all()
        return st

    assert call(np_=-1) == B and call(pr=None) == B
    assert call(cap=0) == B and call(cap=-3) == B and call(cap=65536) == U
    assert call(np_=0) == OK and call(np_=0, cap=0) == B and call(np_=0, cap=65536) == U     # nothing to do, cap still checked
    assert call(nf=0) == B and call(npool=-1) == B and call(nl=0) == B
    for name in ("w", "k", "c", "pt", "cam", "sig", "T", "o", "n"):
        assert call(**{name: None}) == B, name
    prob[1].frame = 1; assert call() == B
    prob[1].frame = -1; assert call() == B
    prob[1].frame = 0
    prob[1].npoints = -1; assert call() == B
    prob[1].npoints = len(idx[1])
    keep = int(idx[1][2])
    idx[1][2] = len(b["world"]); assert call() == B                   # an index outside the pool
    idx[1][2] = -1; assert call() == B
    idx[1][2] = keep
    assert call(npool=keep) == B
    # what host rows allow: a position outside the list, an octave outside [0, nlevels) on a feature with a point
    feat = int(np.nonzero(b["point"][1, :16] >= 0)[0][0])
    pt = b["point"].copy(); pt[1, feat] = len(idx[1]); assert call(pt=pt) == B
    for bad in (8, -1):
        keys["octave"][0, feat] = bad; assert call() == B
    nop = int(np.nonzero(b["point"][0, :16] < 0)[0][0])
    keys["octave"][0, feat] = s["keys"]["octave"][feat]
    pt = b["point"].copy(); pt[1, nop] = -1
    keys["octave"][0, nop] = 99                                       # no point there in either problem: the octave is not read
    assert L.orbx_pose_optimization_batch_device(None, 0, None, 0, None, 0, None, None, None, 16, None, None, 0.0, None, 8, None, None,
                                                 None) == B
    assert call(pt=pt) == OK and (n >= 0).all() and (T != ps.PREFILL_T).any()
    assert call(ur=None) == OK                                        # all monocular
    # the single-call form and the Python mirror raise what the C call returns
    assert _status(lambda: single(host, s, inv_level_sigma2=ps.INV_SIGMA2[:3])) == B
    assert _status(lambda: single(host, s, point=np.where(s["point"] >= 0, len(s["world"]), -1))) == B
    assert _status(lambda: optimizer.pose_optimization_batch(host, [dict(frame=3, Tcw=np.eye(4))], b["world"], 1, keys, None, b["counts"],
                                                             16, b["point"], ps.CAMERA4, ps.MBF, ps.INV_SIGMA2, T, o, n)) == B


# ----------------------------------------------------------------------------------------------- the sin / cos primitive
def test_sin_cos_primitive_close_to_libm(built_lib):
    """largest difference from this machine's libm over the range a tracking update can take, theta in [1e-5, pi], and beyond"""
    import ctypes as C
    L = _capi.lib()
    s, c = C.c_double(), C.c_double()
    rng = np.random.default_rng(0)
    th = np.concatenate([np.geomspace(1e-5, np.pi, 20000), rng.uniform(1e-5, np.pi, 20000), rng.uniform(np.pi, 1e4, 5000)])
    worst = 0.0
    for t in th:
        L.orbx_pose_sin_cos(float(t), C.byref(s), C.byref(c))
        worst = max(worst, abs(s.value - np.sin(t)), abs(c.value - np.cos(t)))
    print("largest |difference| from libm:", worst)
    assert worst <= 2 ** -52                                          # two units in the last place of a value near 1
    for t, (es, ec) in ((0.0, (0.0, 1.0)), (2.0 ** 30, (0.0, 1.0)), (float("nan"), (0.0, 1.0)), (float("inf"), (0.0, 1.0))):
        L.orbx_pose_sin_cos(t, C.byref(s), C.byref(c))
        assert (s.value, c.value) == (es, ec)


# ----------------------------------------------------------------------------------------------- the kernel in the code object
def test_kernel_has_no_scratch_and_calls_no_math_library(built_lib):
    from test_abi import _device_disassembly
    from test_pipeline_room import _kernel_metadata
    meta = _kernel_metadata(built_lib)
    hits = [v for k, v in meta.items() if "k_pose_opt" in k]
    assert len(hits) == 1
    assert int(hits[0]["private_segment_fixed_size"]) == 0
    assert int(hits[0]["group_segment_fixed_size"]) <= 16 * 1024
    m = re.search(r"<_Z\d+k_pose_opt[^>]*>:\n(.*?)s_endpgm", _device_disassembly(built_lib), re.S)
    assert m
    body = m.group(1)
    for op in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64", "v_rsq_f64", "v_fma_f64"):
        assert op in body, op
    assert "v_sqrt_f64" not in body and "s_swappc" not in body and "v_sin" not in body and "v_cos" not in body


# ----------------------------------------------------------------------------------------------- sanitizers
def test_host_unit_clean_under_asan_ubsan(tmp_path):
    """csrc/orbx_pose.cpp (validation, packing, the host path; HIP-free) built with g++ -fsanitize=address,undefined together
    with tests/san_pose_pack.cpp: the size list, index lists, shared frames, every rejection, inputs outside the contract"""
    exe = str(tmp_path / "san_pose_pack")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_pose_pack.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_pose.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr
