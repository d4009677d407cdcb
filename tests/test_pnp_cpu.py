"""PnPsolver RANSAC (orbx_pnp_ransac_batch_create and the cursor calls), the part that needs no GPU: the library's host path
through the C ABI against tests/pnp_model.py, bit for bit -- the double R and t as uint64, the float Tcw as uint32, the chosen N,
counts, masks, every iterate return and the best state after every call -- in both fp_modes; planted scenes with a known pose;
the edges of the RANSAC control; validation before any work; soundness of the poses returned through Refine; the distance of
the library's primitives from LAPACK's; SetRansacParameters; the HIP-free unit under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/san_pnp.cpp, a stand-alone program); no scratch in the two kernels.

The contract is device = host path = model.  Parity with an OpenCV build is not pinned.

Accuracy.  tests/pnp_model.py evaluates the same source with numpy.linalg (eigh, inv, lstsq, svd) in place of the library's
primitives, the stand-in for an OpenCV build.  Two figures are recorded, both measured on the CPU over the
planted scenes, and the test asserts four times each; the scenes are fixed, so the margin only absorbs another libm or LAPACK.
(a) The Refine poses (24 to 55 points: the null space of MtM is one vector, nothing is left to the eigen-solver's rounding):
    |R - R_lapack| <= 2.722e-8, |t - t_lapack| <= 1.598e-7.  This is the distance of the library's primitives from LAPACK's.
(b) The 4-point hypotheses.  With four points MtM has rank 8 at most, and the four rows of ut that compute_ccs reads are
    whatever basis of the null space the eigen-solver's rounding picks; the three beta approximations depend on that basis, so
    after five gauss_newton rounds the two variants sit at different distances from the minimum, or in different minima.  No
    minimal set is well conditioned in that sense, so the rule selects the hypotheses for which the question has an answer: the
    four drawn points are planted inliers and BOTH variants count every planted inlier.  Over those 19 hypotheses
    |R - R_lapack| <= 1.517e-3, |t - t_lapack| <= 2.727e-2, with either variant the one nearer the planted pose: it is the
    spread of 4-point EPnP itself, which the reference has too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pnp_model as pm
import pnp_scenes as ps
from orb_slam2_detailed_comments_amd import (ORBextractor, OrbxError, PnPRansac, _capi, pnp_ransac_parameters,
                                             relocalization_round_robin)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
R_MEASURED, T_MEASURED = 2.722e-8, 1.598e-7      # (a) the Refine poses
R4_MEASURED, T4_MEASURED = 1.517e-3, 2.727e-2    # (b) the 4-point hypotheses


@pytest.fixture(scope="module", params=[_capi.FP_GCC_FMA, _capi.FP_STRICT], ids=["fma", "strict"])
def host(request, built_lib):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2, fp_mode=request.param)
    yield ex
    ex.close()


def run(host, problems, schedule=None, what=""):
    rb = PnPRansac(host, problems)
    try:
        ps.assert_batch_equals_model(rb, problems, what)
        return ps.assert_replay_equals_model(rb, problems, schedule, what)
    finally:
        rb.close()


# ----------------------------------------------------------------------------------------------- planted scenes
def test_planted_scenes_equal_the_model(host):
    problems = list(ps.planted_scenes())
    assert any(p["plane"] for p in problems) and any(np.array_equal(p["truth"], np.eye(4)) for p in problems)
    assert all(len(np.unique(p["max_err"])) == 8 for p in problems)          # octaves 0 .. 7
    for p in problems:
        bad = ~p["planted_inlier"]
        if bad.any():                                           # planted outliers are displaced by 50 px or more
            assert np.linalg.norm(p["p2d"][bad] - ps.project(p["truth"], p["p3dw"])[bad], axis=1).min() >= 49.9
        assert np.abs(p["p2d"][~bad] - ps.project(p["truth"], p["p3dw"])[~bad].astype(F)).max() == 0
    solvers = run(host, problems, what="planted")
    assert all(sv.best is not None for sv in solvers)


def test_round_robin_over_three_solvers_with_iterate_5(host):
    problems = [ps.planted_scenes()[k] for k in (1, 2, 4)]
    rb = PnPRansac(host, problems)
    models = [ps.solver(p) for p in problems]
    rejected = []

    class Model:
        def __len__(self):
            return 3

        def iterate(self, k, n, draw=None):
            return models[k].iterate(n)

    def accept(k, T, inl, nin):                                # PoseOptimization rejects the first answer of every solver
        if k in rejected:
            return k == 2
        rejected.append(k)
        return False

    got = relocalization_round_robin(rb, accept, 5)
    rejected.clear()
    want = relocalization_round_robin(Model(), accept, 5)
    assert got == want and got[0] == 2
    assert sum(1 for k, ret, _, _ in got[1] if k == 2 and ret) == 2          # solver 2 was iterated again after the rejection
    rb.close()


# ----------------------------------------------------------------------------------------------- the RANSAC control
def test_fewer_correspondences_than_min_inliers_is_no_more_at_once(host):
    p = ps.make(20, 8, 0.0, iterations=7, min_inliers=10)
    rb = PnPRansac(host, [p, ps.variant(p, sets=None)])        # the sets of such a problem are not read
    for k in (0, 1):
        assert len(rb.counts(k)) == 0
        r, T, no_more, inl, nin = rb.iterate_raw(k, 5)
        assert r == 0 and no_more and nin == 0 and not inl.any()
        with pytest.raises(OrbxError):
            rb.best(k)
    rb.close()
    assert ps.solver(p).iterate(5)[:2] == (None, True)


def test_min_inliers_equal_to_n_is_one_iteration_and_the_fall_through_return(host):
    """min_inliers == N: SetRansacParameters gives ONE iteration; a count of N qualifies but Refine's strict > can never hold, so
    no Refine succeeds and the fall-through returns mBestTcw with bNoMore"""
    p = ps.make(21, 10, 0.0)
    assert (p["min_inliers"], p["iterations"]) == (10, 1)
    sv = ps.solver(p)
    good = next(s for s in pm.Lcg(21).draw(10, 30) if sv._eval(s).count == 10)
    p = ps.variant(p, sets=np.array([good], np.int32))
    sv = run(host, [p], schedule=[(0, 1)], what="min == N")[0]
    assert sv.done == 1 and sv.best_inliers == 10
    rb = PnPRansac(host, [p])
    assert rb.iterate_raw(0, 5)[0] == -2                       # the loop's OR: iterate(5) wants five iterations, one was drawn
    r, T, no_more, inl, nin = rb.iterate_raw(0, 1)
    assert r == 1 and no_more and nin == 10 and inl.all()
    assert np.array_equal(ps.bits(T.reshape(-1)), ps.bits(sv.best.Tcw.reshape(-1)))     # mBestTcw, not a refined pose
    rb.close()


def test_first_refine_fails_and_a_later_one_succeeds(host):
    p = ps.two_pose_scene()
    sv = ps.solver(p)
    assert sv.hyp(0).count == 12 and sv.hyp(1).count == 30
    assert sv._eval(np.flatnonzero(sv.hyp(0).mask)).count == 12            # Refine of the first best: 12, not more than 12
    sv = run(host, [p], schedule=[(0, 1)], what="two poses")[0]
    assert sv.done == 2 and sv.best_it == 1                     # the call went on past the failed Refine and returned at iteration 1
    rb = PnPRansac(host, [p])
    r, T, no_more, inl, nin = rb.iterate_raw(0, 1)
    assert r == 1 and not no_more and nin == 30 and (inl == p["planted_inlier"]).all()
    rb.close()


def test_iterate_again_after_a_refine_return_before_and_past_max_its_with_append(host):
    """after a return through Refine the solver is called again (PoseOptimization rejected the answer): before mRansacMaxIts it
    goes on; past it the loop's OR still runs n more iterations, which were never drawn: -2, state unchanged, append, again"""
    p = ps.planted_scenes()[1]
    sv = run(host, [p], schedule=[(0, 5)] * 25, what="again")[0]
    assert sv.done > p["iterations"] and len(sv.sets) > p["iterations"]     # the schedule ran past mRansacMaxIts through -2
    rb = PnPRansac(host, [p])
    through_refine = 0
    for _ in range(p["iterations"] + 2):                       # every call returns a pose until the stored iterations run out
        r, T, no_more, inl, nin = rb.iterate_raw(0, 5)
        if r == -2:
            break
        assert r == 1
        through_refine += not no_more                          # a return through Refine leaves bNoMore false
    assert r == -2 and through_refine > 1
    state = (rb.counts(0).copy(), rb.best(0))
    assert rb.iterate_raw(0, 5)[0] == -2                       # and again: nothing has moved
    assert np.array_equal(rb.counts(0), state[0]) and rb.best(0)[1:] == state[1][1:]
    with pytest.raises(RuntimeError):
        rb.iterate(0, 5)                                       # the Python wrapper without a draw callback says so
    rb.close()


def test_append_gives_the_state_of_a_batch_created_with_the_longer_set_list(host):
    p = ps.planted_scenes()[2]
    short = ps.variant(p, sets=p["sets"][:9], iterations=9)
    a, b = PnPRansac(host, [short]), PnPRansac(host, [p])
    a.append(0, p["sets"][9:20])
    a.append(0, p["sets"][20:])
    a.append(0, np.zeros((0, 4), np.int32))
    assert np.array_equal(a.counts(0), b.counts(0)) and len(a.counts(0)) == len(p["sets"])
    for i in range(len(p["sets"])):
        ha, hb = a.hypothesis(0, i), b.hypothesis(0, i)
        assert all(np.array_equal(ps.bits(x), ps.bits(y)) for x, y in zip(ha[:2], hb[:2])) and ha[2] == hb[2] and (ha[3] == hb[3]).all()
    b.close()
    # mRansacMaxIts stays 9: the replay is that of a solver with 9 iterations that was handed further draws
    ps.assert_replay_equals_model(a, [ps.variant(p, iterations=9)], [(0, 5)] * 4, "appended")
    a.close()


def test_set_ransac_parameters(built_lib):
    for n in range(4, 401):
        assert pnp_ransac_parameters(n, **ps.RELOC) == pm.set_ransac_parameters(n, **ps.RELOC), n
        if n >= 20:
            assert pnp_ransac_parameters(n, **ps.RELOC) == (n // 2, 35), n
    for n in (0, 1, 3, 4, 7, 8, 9, 19, 33, 100, 1000, 100000):
        for mi in (4, 8, 10, 50):
            for prob in (0.99, 0.5, 1.0, 0.0):
                for mx in (300, 5, 1, 0):
                    for eps in (0.4, 0.5, 0.0, 1.0):
                        kw = dict(probability=prob, min_inliers=mi, max_iterations=mx, min_set=4, epsilon=eps)
                        assert pnp_ransac_parameters(n, **kw) == pm.set_ransac_parameters(n, **kw), (n, kw)


# ----------------------------------------------------------------------------------------------- sizes, batches
def test_size_list_and_mixed_call(host):
    probs = list(ps.size_problems())
    run(host, probs, what="sizes")
    run(host, list(ps.chunk_problems()), what="LDS chunks")
    mixed = ps.mixed_call()
    run(host, mixed, what="mixed")
    for k, p in enumerate(mixed):                              # batch = single calls
        run(host, [p], what=f"single {k}")
    rb = PnPRansac(host, [])
    assert len(rb) == 0
    rb.close()


# ----------------------------------------------------------------------------------------------- outside the contract
def test_poisoned_input_runs_the_same_code(host):
    probs = list(ps.poisoned())
    assert len(probs) == 8                                      # inf, nan, 1e30, 0.0 in a drawn point and in an undrawn point
    run(host, probs, what="poisoned")
    sv = ps.solver(probs[2])                                    # nan in a drawn point: the hypothesis is non-finite, stored canonically
    h = sv.hyp(0)
    assert np.isnan(h.R).all() and h.count == 0
    assert (ps.bits(h.Tcw[:3].reshape(-1)) == 0x7fc00000).all() and (ps.bits(h.R.reshape(-1)) == 0x7ff8000000000000).all()
    und = ps.solver(probs[3])                                   # nan in an undrawn point: that point is an outlier, nothing else moves
    base = ps.solver(ps.make(140, 24, 0.2, iterations=6, min_inliers=8))
    assert np.array_equal(ps.bits(und.hyp(0).R), ps.bits(base.hyp(0).R))
    bad = int(np.flatnonzero(np.isnan(probs[3]["p3dw"]).any(axis=1))[0])
    assert not any(und.hyp(i).mask[bad] for i in range(6))


# ----------------------------------------------------------------------------------------------- validation
def test_validation_before_any_work(host):
    L, B, OK = _capi.lib(), _capi.BAD_ARGUMENT, _capi.OK
    p = ps.make(50, 12, 0.0, iterations=4, min_inliers=6)
    arr = (_capi.PnpProblem * 2)()
    keep = [np.ascontiguousarray(p[k]) for k in ("p3dw", "p2d", "max_err")] + [p["sets"].copy()]

    def fill():
        for a in arr:
            a.n = 12
            a.p3dw, a.p2d, a.max_err = (v.ctypes.data for v in keep[:3])
            a.camera[:] = list(ps.CAMERA)
            a.min_inliers, a.iterations, a.sets = 6, 4, keep[3].ctypes.data

    def call(n=2, pr=arr, h=host.handle, out=True):
        b = C.c_void_p()
        st = L.orbx_pnp_ransac_batch_create(h, n, C.cast(pr, C.c_void_p) if pr is not None else None, C.byref(b) if out else None)
        if st == OK:
            L.orbx_pnp_batch_destroy(b)
        return st

    fill()
    assert call() == OK
    assert call(n=-1) == B and call(pr=None) == B and call(h=None) == B and call(out=False) == B
    assert call(n=0, pr=None) == OK
    for field, value in (("n", -1), ("iterations", 0), ("p3dw", None), ("p2d", None), ("max_err", None), ("sets", None)):
        fill()
        setattr(arr[1], field, value)
        assert call() == B, field
    for bad in (12, -1):
        fill()
        keep[3][2, 1] = bad
        assert call() == B, bad
        keep[3][:] = p["sets"]
    fill()
    keep[3][3, 2] = keep[3][3, 0]                              # an index repeated within its set: the reference's draw cannot repeat
    assert call() == B
    assert b"repeated" in L.orbx_last_error()
    keep[3][:] = p["sets"]
    fill()
    arr[1].n, arr[1].p3dw, arr[1].sets = 0, None, None          # n == 0 < min_inliers: nothing is read
    assert call() == OK
    rb = PnPRansac(host, [p])
    inl, T = np.zeros(12, np.uint8), np.zeros(16, F)
    nm, ni = C.c_int32(0), C.c_int32(0)
    args = (C.byref(nm), inl.ctypes.data, C.byref(ni), T.ctypes.data)
    assert L.orbx_pnp_batch_iterate(rb._b, 1, 5, *args) == -1 and L.orbx_pnp_batch_iterate(rb._b, -1, 5, *args) == -1
    assert L.orbx_pnp_batch_iterate(None, 0, 5, *args) == -1
    assert L.orbx_pnp_batch_iterate(rb._b, 0, 5, None, inl.ctypes.data, C.byref(ni), T.ctypes.data) == -1
    assert L.orbx_pnp_batch_iterate(rb._b, 0, 5, C.byref(nm), None, C.byref(ni), T.ctypes.data) == -1
    assert L.orbx_pnp_batch_iterate(rb._b, 0, 5, C.byref(nm), inl.ctypes.data, C.byref(ni), None) == -1
    assert L.orbx_pnp_batch_hypothesis(rb._b, 0, 4, None, None, None, None) == B
    assert L.orbx_pnp_batch_hypothesis(rb._b, 0, 3, None, None, None, None) == OK
    s = np.array([[0, 1, 2, 12]], np.int32)
    assert L.orbx_pnp_batch_append(rb._b, 0, 1, s.ctypes.data) == B and L.orbx_pnp_batch_append(rb._b, 0, 1, None) == B
    s[0, 3] = 1
    assert L.orbx_pnp_batch_append(rb._b, 0, 1, s.ctypes.data) == B and L.orbx_pnp_batch_append(rb._b, 0, -1, s.ctypes.data) == B
    assert L.orbx_pnp_batch_append(rb._b, 3, 1, s.ctypes.data) == B
    assert len(rb.counts(0)) == 4                               # none of the rejected calls appended anything
    rb.close()
    small = PnPRansac(host, [ps.make(20, 8, 0.0, iterations=7, min_inliers=10)])
    s[0] = (0, 1, 2, 3)
    assert L.orbx_pnp_batch_append(small._b, 0, 1, s.ctypes.data) == B          # a solver with n < min_inliers has no iterations
    small.close()


# ----------------------------------------------------------------------------------------------- soundness, accuracy
def _refine_return(sv, p):
    r = sv.iterate(p["iterations"])
    assert r is not None and r[0] is not None and not r[1], "not returned through Refine"
    return r


def test_poses_returned_through_refine_separate_the_planted_inliers_from_the_outliers(host):
    """the reference's own test (error2 < mvMaxError) on the returned pose: every planted inlier passes, no planted outlier
    does.  The LAPACK variant is asked first: a scene it cannot solve would say nothing about the library."""
    problems = [p for p in ps.planted_scenes() if p["planted_inlier"].mean() >= 0.5]
    assert len(problems) == 5
    for k, p in enumerate(problems):
        T, _, inl, nin = _refine_return(ps.solver(p, pm.Lapack), p)
        assert (inl == p["planted_inlier"]).all(), ("LAPACK variant", k)
    rb = PnPRansac(host, problems)
    for k, p in enumerate(problems):
        r, T, no_more, inl, nin = rb.iterate_raw(k, p["iterations"])
        assert r == 1 and not no_more, k                        # through Refine
        assert (inl == p["planted_inlier"]).all() and nin == p["planted_inlier"].sum(), k
        R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
        assert (pm.check_inliers(R, t, p["camera"], p["p3dw"], p["p2d"], p["max_err"]) == p["planted_inlier"]).all(), k
        assert np.abs(T - p["truth"]).max() < 1e-3, k          # and it is the planted pose
    rb.close()


def test_distance_from_the_lapack_variant(built_lib):
    worst = {"refine": [0.0, 0.0], "minimal": [0.0, 0.0]}
    used = {"refine": 0, "minimal": 0}
    for p in ps.planted_scenes():
        own, lap = ps.solver(p), ps.solver(p, pm.Lapack)
        _refine_return(own, p), _refine_return(lap, p)
        pairs = [("refine", own.refine(), lap.refine())]       # (a) the Refine poses
        for i, s in enumerate(own.sets):                        # (b) 4-point hypotheses where both reach the planted pose
            if p["planted_inlier"][list(s)].all():
                ho, hl = own.hyp(i), lap.hyp(i)
                if (ho.mask | ~p["planted_inlier"]).all() and (hl.mask | ~p["planted_inlier"]).all():
                    pairs.append(("minimal", ho, hl))
        for kind, ho, hl in pairs:
            worst[kind][0] = max(worst[kind][0], float(np.abs(ho.R - hl.R).max()))
            worst[kind][1] = max(worst[kind][1], float(np.abs(ho.t - hl.t).max()))
            used[kind] += 1
    for kind in worst:
        print(f"{kind}: {used[kind]} compared; largest |R - R_lapack| = {worst[kind][0]:.3e}, |t - t_lapack| = {worst[kind][1]:.3e}")
    assert used["refine"] == len(ps.planted_scenes()) and used["minimal"] >= used["refine"]
    assert worst["refine"][0] <= 4 * R_MEASURED and worst["refine"][1] <= 4 * T_MEASURED
    assert worst["minimal"][0] <= 4 * R4_MEASURED and worst["minimal"][1] <= 4 * T4_MEASURED


# ----------------------------------------------------------------------------------------------- sanitizers
def test_host_unit_clean_under_asan_ubsan(tmp_path):
    """csrc/orbx_pnp.cpp (validation, packing, the host path, Refine, the cursor, append; HIP-free) built with g++
    -fsanitize=address,undefined together with tests/san_pnp.cpp, a stand-alone program: sizes around the mask words, every
    rejection, replays that run past the stored iterations, degenerate and non-finite input"""
    exe = str(tmp_path / "san_pnp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_pnp.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_pnp.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr


# ----------------------------------------------------------------------------------------------- the kernels in the code object
def test_kernels_have_no_scratch_and_fit_the_lds(built_lib):
    from test_pipeline_room import _kernel_metadata
    meta = _kernel_metadata(built_lib)
    for name, lds in (("k_pnp_hypotheses", (496 + 12 * 4) * 32 * 8), ("k_pnp_inliers", 6 * 512 * 4)):
        hits = [v for k, v in meta.items() if name in k]
        assert len(hits) == 1, name
        assert int(hits[0]["private_segment_fixed_size"]) == 0, name
        assert int(hits[0]["group_segment_fixed_size"]) == lds and lds <= 160 * 1024, name
