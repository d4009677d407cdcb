"""Optimizer::LocalBundleAdjustment (orbx_local_bundle_adjustment_batch), the part that needs no GPU: the library's host path
through the C ABI on a host-only handle against tests/localba_model.py, bit for bit on the pose and point floats, the erase
bytes, the iteration counts and the chi2 doubles; the size list; the special scenes; inputs outside the contract; validation
before any work; sanity checks of the model itself (the Schur step against a dense solve of the full system, truth recovery,
chi2 monotone, planted outliers erased); the HIP-free unit under AddressSanitizer + UndefinedBehaviorSanitizer
(tools/san_localba.cpp, a stand-alone program).

The contract is device = host path = model.  Parity with a g2o + Eigen build is not pinned."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import localba_cases as cases
import localba_model as lm
import localba_scenes as sc
from orb_slam2_detailed_comments_amd import ORBextractor, OrbxError, _capi, localmapping, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(built_lib):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    yield ex
    ex.close()


# ----------------------------------------------------------------------------------------------- host path == model
def test_size_list_host_path_equals_model(host):
    scenes = cases.size_scenes()
    assert {(s["nlocal"], len(s["Tcw"]) - s["nlocal"], len(s["world"])) for s in scenes} >= {(1, 0, 1), (2, 0, 64), (2, 5, 65), (3, 1, 257)}
    edges_of = lambda s, k: int(np.sum(s["obs_kf"] == k))
    assert [edges_of(scenes[i], k) for i, k in ((8, 0), (9, 1), (10, 2), (11, 0))] == [63, 64, 65, 129]
    deg = np.diff(scenes[6]["obs_begin"])
    assert deg.min() == 2 and deg.max() == 17                  # observations per point from 2 up to all keyframes
    cases.assert_all(host, dict(enumerate(scenes)))
    big = cases.model(scenes[7])[0]                            # 66 local keyframes: the vertex chains wrap
    assert big["iters"][0] >= 1 and big["iters"][1] == 0


def test_special_scenes_host_path_equals_model(host):
    named = cases.special_scenes()
    cases.assert_all(host, named)
    mo = {n: cases.model(p) for n, p in named.items()}
    # a locally fixed keyframe gets the quaternion round trip of its input, not its input
    p = named["local_fixed"]
    assert np.abs(mo["local_fixed"][0]["Tcw"][1] - p["Tcw"][1]).max() < 1e-6
    assert not np.array_equal(mo["local_fixed"][0]["Tcw"][0], p["Tcw"][0])
    assert mo["one_round"][0]["iters"][1] == 0 and mo["one_round"][0]["nflagged"] == 0
    assert mo["gauge_free"][0]["iters"][0] == 5                # the damping alone makes the free gauge solvable
    for seed in cases.DEPTH_SEEDS:                             # isDepthPositive alone flags an edge
        r1 = [t for t in mo["depth_%d" % seed][1] if t[0] == "round1"][0]
        assert r1[2] > 0, seed
    # a flagged edge whose final chi2 is the stale one: judged afresh at the final estimates, its answer would differ
    assert [t for t in mo["local_fixed"][1] if t[0] == "final"][0][1] > 0 or \
        [t for t in cases.model(cases.size_scenes()[6])[1] if t[0] == "final"][0][1] > 0


def test_rejected_last_trial_and_the_stale_error_rule(host):
    """e->chi2() is the error of the last computeActiveErrors, which is the last TRIAL, accepted or not; isDepthPositive reads the
    current estimates.  Inside the contract a round ends on a rejected trial only at the convergence floor (ten rejections in a
    row, or rho == 0): of 670 searched scenes (noisy and perturbed, noise free, started at the truth) none ended round 1 that
    way within its five iterations, and at the floor a rejected trial differs from the estimate by rounding only.  The scene
    that pins the rule through the full run has a point seen only by fixed keyframes with a NaN coordinate: the reduced system
    stays finite and is solved, chi2 is NaN, so EVERY trial of round 1 is rejected, the estimates do not move, and the errors the
    classification reads are those one Gauss-Newton step away from them -- there the rule decides flags.  The debug entry point
    (test_classification_alone) pins it for arbitrary pairs of estimates."""
    nanp = cases._only(sc.make(52, 3, 3, 40, min_obs=6, noise=0.7, perturb=(0.1, 0.05, 0.2)), "split")
    nanp["world"] = nanp["world"].copy(); nanp["world"][0, 2] = np.nan
    cases.assert_all(host, {"nan": nanp})
    mo, tr = cases.model(nanp)
    trials = [t for t in tr if t[0] == "trial" and t[1]]
    assert len(trials) == 5 and all(not t[3] and t[4] for t in trials)   # round 1: every trial rejected, every solve succeeded
    assert [t for t in tr if t[0] == "round1"][0][1] > 0, "the stale-error rule decides at least one flag"
    assert mo["iters"][1] >= 1                                 # the NaN point's edges fail the depth test and leave: round 2 runs


def test_outside_the_contract_host_path_equals_model(host):
    named = cases.outside_scenes()
    cases.assert_all(host, named)
    for n, p in named.items():
        mo = cases.model(p)[0]
        assert 0 <= mo["iters"][0] <= 5 and 0 <= mo["iters"][1] <= 10, n


def test_classification_alone(host):
    dc = cases.debug_cases()
    got = optimizer.debug_localba_classify(host, [d[0] for d in dc], [(d[1][0], d[1][1], d[2][0], d[2][1]) for d in dc])
    for k, ((p, est, last), (erase, info)) in enumerate(zip(dc, got)):
        want = lm.classify(p, est[0], est[1], last[0], last[1])
        assert np.array_equal(erase, want), k
        assert int(info["nerase"]) == int(want.sum())
    # swapping est and last changes the answer: the chi2 is taken at `last`
    assert not np.array_equal(got[0][0], got[1][0])
    # the mirrored point: chi2 at `last` (the truth) is ~0, the depth at the estimate is negative -- the depth test alone
    p = dc[-1][0]
    e0 = np.nonzero((np.repeat(np.arange(len(p["world"])), np.diff(p["obs_begin"])) == 0) & (p["obs_kf"] == 0))[0]
    assert len(e0) == 1 and got[-1][0][e0[0]] == 1 and got[-1][0].sum() >= 1


def test_batches_and_empty_call(host):
    scenes = list(cases.size_scenes()[:6])
    one = [optimizer.local_bundle_adjustment_batch(host, [s])[0] for s in scenes]
    many = optimizer.local_bundle_adjustment_batch(host, scenes)
    for a, b, s in zip(one, many, scenes):
        cases.assert_equal(a, cases.model(s)[0], "alone")
        cases.assert_equal(b, cases.model(s)[0], "in a batch")
    assert optimizer.local_bundle_adjustment_batch(host, []) == []
    assert _capi.lib().orbx_local_bundle_adjustment_batch(host.handle, 0, None, None) == _capi.OK


def test_streams_in_lock_step_are_one_call(host):
    """localmapping.local_bundle_adjustment_rounds: the streams' problems in one call, a stream whose stop flag is set skipped"""
    scenes = cases.size_scenes()
    streams = [scenes[2], None, scenes[4], scenes[5]]
    out = localmapping.local_bundle_adjustment_rounds(host, streams, refresh=False)
    assert out[1] is None
    for s, r in zip(streams, out):
        if s is not None:
            cases.assert_equal((r["Tcw"], r["world"], r["erase"], r["info"]), cases.model(s)[0], "stream")
    assert localmapping.local_bundle_adjustment_rounds(host, [None, None]) == [None, None]


def _prefilled(p):
    q = dict(p)
    q["Tcw_out"] = np.full((p["nlocal"], 16), 7.5, np.float32)
    q["world_out"] = np.full((len(p["world"]), 3), 7.5, np.float32)
    q["erase"] = np.full(len(p["obs_kf"]), 9, np.uint8)
    return q


def test_validation_before_any_work(host):
    good = cases.size_scenes()[1]
    bad = []
    q = _prefilled(good); q["obs_begin"] = q["obs_begin"].copy(); q["obs_begin"][3] = q["obs_begin"][2] - 1; bad.append((q, _capi.BAD_ARGUMENT))
    q = _prefilled(good); q["obs_begin"] = q["obs_begin"].copy(); q["obs_begin"][0] = 1; bad.append((q, _capi.BAD_ARGUMENT))
    q = _prefilled(good); q["obs_kf"] = q["obs_kf"].copy(); q["obs_kf"][4] = 2; bad.append((q, _capi.BAD_ARGUMENT))
    q = _prefilled(good); q["obs_kf"] = q["obs_kf"].copy(); q["obs_kf"][4] = -1; bad.append((q, _capi.BAD_ARGUMENT))
    q = _prefilled(good); q["obs_kf"] = q["obs_kf"].copy(); q["obs_kf"][1] = q["obs_kf"][0]; bad.append((q, _capi.BAD_ARGUMENT))
    big = _prefilled(sc.make(61, 129, 1, 3, max_obs=3)); bad.append((big, _capi.UNSUPPORTED))
    for q, code in bad:
        first = _prefilled(good)                               # a good problem ahead of the bad one is not run either
        with pytest.raises(OrbxError) as err:
            optimizer.local_bundle_adjustment_batch(host, [first, q])
        assert err.value.status == code, str(err.value)
        for r in (first, q):
            assert (r["Tcw_out"] == 7.5).all() and (r["world_out"] == 7.5).all() and (r["erase"] == 9).all()
    assert "128" in str(err.value)                             # the limit is named
    L = _capi.lib()
    res = np.zeros(1, _capi.LOCALBA_RESULT_DTYPE)
    arr, hold, outs = optimizer._localba_marshal([_prefilled(good)])
    assert L.orbx_local_bundle_adjustment_batch(host.handle, -1, C.cast(arr, C.c_void_p), res.ctypes.data) == _capi.BAD_ARGUMENT
    assert L.orbx_local_bundle_adjustment_batch(host.handle, 1, None, res.ctypes.data) == _capi.BAD_ARGUMENT
    assert L.orbx_local_bundle_adjustment_batch(host.handle, 1, C.cast(arr, C.c_void_p), None) == _capi.BAD_ARGUMENT
    for field in ("Tcw", "local_fixed", "world", "obs_begin", "obs_kf", "obs", "inv_sigma2", "Tcw_out", "world_out", "erase"):
        arr, hold, outs = optimizer._localba_marshal([_prefilled(good)])
        setattr(arr[0], field, None)
        assert L.orbx_local_bundle_adjustment_batch(host.handle, 1, C.cast(arr, C.c_void_p), res.ctypes.data) == _capi.BAD_ARGUMENT, field
    for field in ("nlocal", "nfixed", "npoints"):
        arr, hold, outs = optimizer._localba_marshal([_prefilled(good)])
        setattr(arr[0], field, -1)
        assert L.orbx_local_bundle_adjustment_batch(host.handle, 1, C.cast(arr, C.c_void_p), res.ctypes.data) == _capi.BAD_ARGUMENT, field


# ----------------------------------------------------------------------------------------------- sanity of the model itself
def test_schur_step_solves_the_full_system():
    """One linearisation of a mid-size scene (6 free keyframes, 120 points: 396 unknowns): the model's Schur step against
    numpy.linalg.solve on the full damped system.  The reference solution is the dense solve refined in np.longdouble until it
    stands still.  Measured on the CPU: the dense solve's own relative error 4.67e-15, the Schur step's 1.14e-14; the Schur step
    is allowed 16 times the dense solve's error (two elimination orders of one well-damped system)."""
    p = sc.make(71, 6, 3, 120, noise=0.5)
    H, b, x = lm.full_system(p)
    assert H.shape[0] == 6 * 6 + 3 * 120
    xd = np.linalg.solve(H, b)
    Hl, bl = H.astype(np.longdouble), b.astype(np.longdouble)
    ref = xd.astype(np.longdouble)
    for _ in range(6):
        ref = ref + np.linalg.solve(H, (bl - Hl @ ref).astype(np.float64)).astype(np.longdouble)
    nrm = float(np.linalg.norm(ref))
    e_dense = float(np.linalg.norm(xd - ref)) / nrm
    e_schur = float(np.linalg.norm(x - ref)) / nrm
    print("dense %.3e schur %.3e" % (e_dense, e_schur))
    assert e_dense > 0 and e_schur <= 16 * e_dense


TRUTH = ((81, 3, 2, 60), (82, 5, 3, 100), (83, 2, 2, 40))


def test_noise_free_scenes_recover_the_true_poses():
    """A convergence check, not a parity check: noise-free mixed scenes with fixed keyframes.  The bound 1e-5 is the one
    tests/test_pose_batch_gpu.py uses on the same scene scale; the model does not meet it within its 5 + 10 iterations: its largest error on
    these seeds (max over the pose entries, float32 poses), measured on the CPU, is 1.82e-5; the bound is four times that."""
    worst = 0.0
    for seed, nl, nf, npt in TRUTH:
        p = sc.make(seed, nl, nf, npt, mode="mixed")
        mo = cases.model(p)[0]
        worst = max(worst, float(np.abs(mo["Tcw"].astype(np.float64) - p["Tcw_true"][:nl]).max()))
        assert mo["nerase"] == 0
    print("worst %.3e" % worst)
    assert worst < TRUTH_BOUND


TRUTH_BOUND = 4 * 1.82e-5


def test_chi2_never_rises_and_planted_outliers_are_erased():
    """20 % gross outliers (12 to 40 level sigmas, so every planted residual exceeds 10 px): the erase list holds every one of
    them; and in every run of this file's scenes the robust chi2 at the end of a round is not above the one it started from."""
    for seed in (93, 94, 97):
        p = sc.make(seed, 5, 3, 120, noise=0.7, outlier_frac=0.2)
        mo = cases.model(p)[0]
        assert p["planted"].sum() > 50 and (p["gross"][p["planted"]] > 10).all()
        assert mo["erase"][p["planted"]].all(), seed
        assert mo["erase"][~p["planted"]].mean() < 0.05
        assert mo["chi2"][1] <= mo["chi2"][0] and mo["chi2"][3] <= mo["chi2"][2]
    for s in list(cases.size_scenes()) + list(cases.special_scenes().values()):
        c = cases.model(s)[0]["chi2"]
        assert c[1] <= c[0] and c[3] <= c[2]


# ----------------------------------------------------------------------------------------------- sanitizers
def test_host_unit_clean_under_asan_ubsan(tmp_path):
    """csrc/orbx_localba.cpp (validation, packing with the derived lists, the host path; HIP-free) built with g++
    -fsanitize=address,undefined together with tools/san_localba.cpp: two scenes and the rejections"""
    exe = str(tmp_path / "san_localba")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "san_localba.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_localba.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr
