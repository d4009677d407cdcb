"""Sim3Solver RANSAC (orbx_sim3_ransac_batch_create and the cursor calls), the part that needs no GPU: the library's host path
through the C ABI against tests/sim3_model.py, bit for bit -- the hypothesis floats as uint32, counts, masks, every iterate
return and the best state after every call -- in both fp_modes; planted scenes with a known Sim3; the edges of the RANSAC
control and of the arithmetic; validation before any work; the accuracy of R against a float64 Horn; SetRansacParameters; the
atan2 primitive; the HIP-free unit under AddressSanitizer + UndefinedBehaviorSanitizer (tests/san_sim3.cpp, a stand-alone
program); no scratch in the two kernels.

The contract is device = host path = model.  Parity with an OpenCV build is not pinned from N to R.

Accuracy.  Over the hypotheses of the planted scenes whose triple spans a triangle of more than AREA_FLOOR m^2 in both frames,
the largest |R - R_float64| measured on the CPU is 1.211e-5 (profiles/sim3_batch.md); the test asserts four times that.  The
margin covers other seeds, not other algorithms."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sim3_model as sm
import sim3_scenes as ss
from orb_slam2_detailed_comments_amd import ORBextractor, OrbxError, Sim3Ransac, _capi, compute_sim3_round_robin, ransac_iterations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
AREA_FLOOR = 0.05
R_MEASURED = 1.211e-5


@pytest.fixture(scope="module", params=[_capi.FP_GCC_FMA, _capi.FP_STRICT], ids=["fma", "strict"])
def host(request, built_lib):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2, fp_mode=request.param)
    yield ex
    ex.close()


def run(host, problems, schedule=None, what=""):
    rb = Sim3Ransac(host, problems)
    try:
        ss.assert_batch_equals_model(rb, problems, what)
        return ss.assert_replay_equals_model(rb, problems, schedule, what)
    finally:
        rb.close()


# ----------------------------------------------------------------------------------------------- planted scenes
def test_planted_scenes_equal_the_model_and_recover_the_planted_inliers(host):
    problems = list(ss.planted_scenes())
    for p in problems:
        assert 0.7 <= p["truth"][0] <= 1.4
        hyps, masks, counts = ss.model(p)
        pure = p["planted_inlier"][p["sets"]].all(axis=1)      # hypotheses from three planted inliers
        assert pure.any()
        assert any((masks[i] | ~p["planted_inlier"]).all() for i in np.nonzero(pure)[0])   # ... one recovers every planted inlier
        assert counts.max() > p["min_inliers"]
    solvers = run(host, problems, what="planted")
    assert all(sv.done == p["iterations"] for sv, p in zip(solvers, problems))


def test_iterations_of_1_5_and_300(host):
    problems = [ss.make(10, 30, iterations=1, min_inliers=6), ss.make(11, 30, iterations=5, min_inliers=6),
                ss.make(12, 100, iterations=300, min_inliers=20)]
    run(host, problems, what="iterations")
    run(host, problems, schedule=[(0, 1), (0, 1), (1, 3), (1, 3), (2, 300), (2, 300), (2, 1)], what="iterations, other calls")


# ----------------------------------------------------------------------------------------------- the RANSAC control
def test_fewer_correspondences_than_min_inliers_is_no_more_at_once(host):
    p = ss.make(20, 10, iterations=7, min_inliers=20)
    assert ss.model(p) is None
    rb = Sim3Ransac(host, [p, ss.variant(p, sets=None)])       # the sets of such a problem are not read
    for k in (0, 1):
        assert len(rb.counts(k)) == 0
        T, no_more, inl, nin = rb.iterate(k, 5)
        assert T is None and no_more and nin == 0 and not inl.any()
        with pytest.raises(OrbxError):
            rb.best(k)
    rb.close()


def test_n_equal_to_min_inliers_gives_one_iteration(host):
    assert ransac_iterations(20, 0.99, 20, 300) == 1 == sm.ransac_iterations(20, 0.99, 20, 300)
    p = ss.make(21, 20, outlier_frac=0.0, min_inliers=20)
    assert p["iterations"] == 1
    sv = run(host, [p], schedule=[(0, 5), (0, 5)])[0]
    assert sv.done == 1 and sv.best_inliers <= 20              # at most n inliers: never more than min_inliers, nothing returned


def test_count_equal_to_min_inliers_is_not_returned_and_best_moves_on_equal_counts(host):
    base = ss.planted_scenes()[3]
    counts = ss.model(base)[2]
    top = int(counts.max())
    where = np.nonzero(counts == top)[0]
    assert len(where) >= 3
    p = ss.variant(base, min_inliers=top)                      # the best count EQUALS min_inliers: not returned
    rb = Sim3Ransac(host, [p])
    sv = sm.Solver(p, ss.model(p))
    seen = []
    for i in range(p["iterations"]):
        T, no_more, inl, nin = rb.iterate(0, 1)
        assert sv.iterate(1)[0] is None and T is None and nin == 0 and no_more == (i == p["iterations"] - 1)
        R, t, s = rb.best(0)
        wR, wt, ws = sv.best()
        assert np.array_equal(ss.bits(R), ss.bits(wR)) and np.array_equal(ss.bits(t), ss.bits(wt)) and ss.bits(s) == ss.bits(ws)
        seen.append(sv.best_it)
    assert [seen[i] for i in where] == list(where)             # every iteration that ties the best takes it over (>=)
    hy = ss.model(p)[0]
    assert not np.array_equal(ss.bits(hy[where[0]]), ss.bits(hy[where[1]]))
    rb.close()


def test_iterate_5_past_a_first_success_and_no_more_on_exhaustion(host):
    p = ss.planted_scenes()[0]
    solvers = run(host, [p])                                   # iterate(5) until exhausted, every return compared
    rb = Sim3Ransac(host, [p])
    hits, calls = 0, 0
    while True:
        T, no_more, inl, nin = rb.iterate(0, 5)
        calls += 1
        hits += T is not None
        if T is not None:
            assert nin == inl.sum() > p["min_inliers"]
        if no_more:
            break
    assert hits >= 2 and calls <= p["iterations"]
    T, no_more, inl, nin = rb.iterate(0, 5)                    # an exhausted solver: nothing, no_more again
    assert T is None and no_more and nin == 0
    rb.close()
    assert solvers[0].done == p["iterations"]


def test_round_robin_replays_the_compute_sim3_loop(host):
    problems = [ss.make(30, 25, iterations=12, min_inliers=20, outlier_frac=0.6), ss.make(31, 10, iterations=4, min_inliers=20),
                ss.planted_scenes()[1], ss.planted_scenes()[2]]
    rb = Sim3Ransac(host, problems)
    solvers = [sm.Solver(p, ss.model(p)) for p in problems]

    class Model:
        def __len__(self):
            return len(solvers)

        def iterate(self, k, n):
            return solvers[k].iterate(n)

    rejected = []

    def accept(k, T, inl, nin):                                # "OptimizeSim3" rejects the first answer of every solver
        if k in rejected:
            return k == 3
        rejected.append(k)
        return False

    got = compute_sim3_round_robin(rb, accept)
    rejected = []
    want = compute_sim3_round_robin(Model(), accept)
    assert got == want and got[0] == 3
    assert any(k == 1 and no_more and not ret for k, ret, no_more, _ in got[1])     # n < min_inliers: discarded at its first call
    assert sum(1 for k, ret, _, _ in got[1] if k == 3 and ret) == 2      # solver 3 was iterated again after the rejection
    rb.close()


def test_set_ransac_parameters(built_lib):
    for n in (0, 1, 3, 19, 20, 21, 25, 40, 100, 1000, 100000):
        for mi in (3, 6, 20):
            for prob in (0.99, 0.5, 1.0, 0.0):
                for mx in (300, 5, 1, 0):
                    assert ransac_iterations(n, prob, mi, mx) == sm.ransac_iterations(n, prob, mi, mx), (n, mi, prob, mx)
    assert ransac_iterations(100, 0.99, 20, 300) == 300 and ransac_iterations(25, 0.99, 20, 300) == 7


# ----------------------------------------------------------------------------------------------- the arithmetic's edges
def test_fix_scale_on_and_off(host):
    a = ss.make(40, 50, iterations=20, min_inliers=10)
    b = ss.variant(a, fix_scale=1)
    run(host, [a, b], what="fix_scale")
    assert (ss.model(b)[0][:, 44] == 1.0).all() and (ss.model(a)[0][:, 44] != 1.0).any()


def test_degenerate_triples_and_points_outside_the_contract(host):
    p = ss.degenerate()
    hyps, masks, counts = ss.model(p)
    assert not np.isfinite(hyps[1][:12]).all() and counts[1] == 0          # |v| = 0: 0 / 0 in the scaling, nothing is an inlier
    assert counts[4] > p["min_inliers"]
    assert not masks[:, 10].any()                              # a non-finite err compares as "not less": outlier
    run(host, [p], what="degenerate")


def test_point_that_lands_on_z_zero_is_an_outlier(host):
    """a correspondence whose X2c the hypothesis maps to z == 0 exactly in camera 1 (found by search: the float row sum cancels)"""
    p = ss.make(42, 30, iterations=3, min_inliers=6, outlier_frac=0.0)
    T = ss.model(p)[0][0][:16].reshape(4, 4)
    free = [i for i in range(30) if i not in set(p["sets"].ravel())][0]
    rng = np.random.default_rng(5)
    found = None
    for _ in range(20000):
        x, y = F(rng.uniform(-1, 1)), F(rng.uniform(-1, 1))
        z = F(-(np.float64(T[2, 0]) * x + np.float64(T[2, 1]) * y + np.float64(T[2, 3])) / np.float64(T[2, 2]))
        if ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3] == 0:
            found = (x, y, z)
            break
    assert found is not None
    x2 = p["x2c"].copy()
    x2[free] = found
    q = ss.variant(p, x2c=x2)
    assert np.array_equal(ss.bits(ss.model(q)[0][0]), ss.bits(ss.model(p)[0][0]))   # the hypothesis does not depend on that point
    assert not ss.model(q)[1][0, free]
    run(host, [q], what="z == 0")


@pytest.mark.parametrize("poison", [np.inf, np.nan, 1e30, 0.0])
def test_non_finite_input_runs_the_same_code(host, poison):
    p = ss.make(43, 24, iterations=8, min_inliers=6)
    x1 = p["x1c"].copy()
    x1[p["sets"][0, 0]] = poison
    x1[p["sets"][3, 1], 2] = poison
    run(host, [ss.variant(p, x1c=x1)], what=str(poison))


# ----------------------------------------------------------------------------------------------- sizes, batches
def test_size_list_and_mixed_call(host):
    probs = list(ss.size_problems())
    for a in range(0, len(probs), 16):
        run(host, probs[a:a + 16], schedule=[(k, 7) for _ in range(3) for k in range(len(probs[a:a + 16]))], what=f"sizes {a}")
    run(host, list(ss.chunk_problems()), what="LDS chunks")
    mixed = ss.mixed_call()
    run(host, mixed, what="mixed")
    for k, p in enumerate(mixed):                              # batch = single calls
        run(host, [p], what=f"single {k}")
    rb = Sim3Ransac(host, [])
    assert len(rb) == 0
    rb.close()


# ----------------------------------------------------------------------------------------------- validation
def test_validation_before_any_work(host):
    L, B, OK = _capi.lib(), _capi.BAD_ARGUMENT, _capi.OK
    p = ss.make(50, 12, iterations=4, min_inliers=6)
    arr = (_capi.Sim3Problem * 2)()
    keep = [np.ascontiguousarray(p[k]) for k in ("x1c", "x2c", "max_err1", "max_err2")] + [p["sets"].copy()]

    def fill():
        for a in arr:
            a.n = 12
            a.x1c, a.x2c, a.max_err1, a.max_err2 = (v.ctypes.data for v in keep[:4])
            a.camera1[:] = ss.CAMERA1.tolist(); a.camera2[:] = ss.CAMERA2.tolist()
            a.fix_scale, a.min_inliers, a.iterations, a.sets = 0, 6, 4, keep[4].ctypes.data

    def call(n=2, pr=arr, h=host.handle):
        b = C.c_void_p()
        st = L.orbx_sim3_ransac_batch_create(h, n, C.cast(pr, C.c_void_p) if pr is not None else None, C.byref(b))
        if st == OK:
            L.orbx_sim3_batch_destroy(b)
        else:
            assert b.value is None                             # nothing is written on failure
        return st

    fill()
    assert call() == OK and call(n=0) == OK and call(n=0, pr=None) == OK
    assert call(n=-1) == B and call(pr=None) == B and call(h=None) == B
    assert L.orbx_sim3_ransac_batch_create(host.handle, 2, C.cast(arr, C.c_void_p), None) == B
    for field in ("x1c", "x2c", "max_err1", "max_err2", "sets"):
        setattr(arr[1], field, None)
        assert call() == B, field
        fill()
    arr[1].n = -1; assert call() == B
    fill()
    for bad in (0, -2):
        arr[1].iterations = bad; assert call() == B
    fill()
    for pos, bad in ((0, 12), (5, -1), (11, 1 << 30)):
        keep[4].ravel()[pos] = bad; assert call() == B
        keep[4][:] = p["sets"]
    keep[4][2] = (3, 3, 3); assert call() == OK               # repeated indices are accepted
    keep[4][:] = p["sets"]
    arr[1].n = 0; arr[1].x1c = None; arr[1].min_inliers = 0; assert call() == B     # n = 0 that launches: every index is outside
    arr[1].min_inliers = 1; arr[1].sets = None; assert call() == OK                 # n < min_inliers: nothing is read
    fill()
    # the cursor calls
    rb = Sim3Ransac(host, [p])
    no_more, nin = C.c_int32(), C.c_int32()
    T, inl = np.full(16, 7, F), np.full(12, 9, np.uint8)
    for k in (-1, 1):
        assert L.orbx_sim3_batch_iterate(rb._b, k, 5, C.byref(no_more), _capi.ptr(inl), C.byref(nin), _capi.ptr(T)) == -1
    assert L.orbx_sim3_batch_iterate(None, 0, 5, C.byref(no_more), _capi.ptr(inl), C.byref(nin), _capi.ptr(T)) == -1
    assert L.orbx_sim3_batch_iterate(rb._b, 0, 5, None, _capi.ptr(inl), C.byref(nin), _capi.ptr(T)) == -1
    assert (T == 7).all() and (inl == 9).all()
    assert L.orbx_sim3_batch_best(rb._b, 0, _capi.ptr(T), _capi.ptr(T), C.byref(C.c_float())) == B      # before the first iteration
    assert L.orbx_sim3_batch_best(rb._b, 1, _capi.ptr(T), _capi.ptr(T), C.byref(C.c_float())) == B
    assert L.orbx_sim3_batch_counts(rb._b, 2, _capi.ptr(T), None) == B
    assert L.orbx_sim3_batch_hypothesis(rb._b, 0, 4, _capi.ptr(T), None) == B
    assert L.orbx_sim3_batch_hypothesis(rb._b, 0, -1, _capi.ptr(T), None) == B
    assert (T == 7).all()
    assert L.orbx_sim3_batch_iterate(rb._b, 0, 0, C.byref(no_more), _capi.ptr(inl), C.byref(nin), _capi.ptr(T)) == 0   # iterate(0): nothing runs
    assert no_more.value == 0 and (inl == 0).all()
    rb.close()
    L.orbx_sim3_batch_destroy(None)


# ----------------------------------------------------------------------------------------------- accuracy
def rotation_differences():
    """|R - R_float64| of every hypothesis of the planted scenes whose triple spans more than AREA_FLOOR in both frames"""
    out = []
    for p in ss.planted_scenes():
        hyps = ss.model(p)[0]
        for i, s in enumerate(p["sets"]):
            a, b = p["x1c"][s].astype(np.float64), p["x2c"][s].astype(np.float64)
            area = min(0.5 * np.linalg.norm(np.cross(m[1] - m[0], m[2] - m[0])) for m in (a, b))
            if area > AREA_FLOOR:
                out.append(np.abs(hyps[i][32:41].reshape(3, 3).astype(np.float64) - sm.horn_float64(a, b)).max())
    return np.array(out)


def test_rotation_against_float64_horn(host):
    d = rotation_differences()
    print("hypotheses", len(d), "largest |R - R_float64|", d.max())
    assert len(d) >= 300
    assert d.max() <= 4 * R_MEASURED
    # the library's R is the model's (asserted bit for bit above); one direct check through the ABI
    p = ss.planted_scenes()[0]
    rb = Sim3Ransac(host, [p])
    h, _ = rb.hypothesis(0, 0)
    assert np.array_equal(ss.bits(h), ss.bits(ss.model(p)[0][0]))
    rb.close()


# ----------------------------------------------------------------------------------------------- the atan2 primitive
def test_atan2_primitive_close_to_libm(built_lib):
    """(|v|, q0) on the unit circle, the arguments ComputeSim3 hands it; tools/sim3_atan2_check.cpp sweeps 2e7 points: 2^-51"""
    L = _capi.lib()
    a = np.concatenate([np.linspace(0, np.pi, 40001), np.random.default_rng(0).uniform(0, np.pi, 20000)])
    worst = max(abs(L.orbx_sim3_atan2(float(abs(np.sin(t))), float(np.cos(t))) - np.arctan2(abs(np.sin(t)), np.cos(t))) for t in a)
    print("largest |difference| from libm:", worst)
    assert worst <= 2 ** -51
    assert L.orbx_sim3_atan2(0.0, 1.0) == 0.0 and L.orbx_sim3_atan2(0.0, 0.0) == 0.0 and L.orbx_sim3_atan2(1.0, 0.0) == np.pi / 2
    assert L.orbx_sim3_atan2(0.0, -1.0) == np.pi and np.isnan(L.orbx_sim3_atan2(float("nan"), 1.0))


# ----------------------------------------------------------------------------------------------- the kernels in the code object
def test_kernels_have_no_scratch_and_call_no_math_library(built_lib):
    from test_abi import _device_disassembly
    from test_pipeline_room import _kernel_metadata
    meta = _kernel_metadata(built_lib)
    dis = _device_disassembly(built_lib)
    for name, lds in (("k_sim3_hypotheses", 0), ("k_sim3_inliers", 12 * 512 * 4)):
        hits = [v for k, v in meta.items() if name in k]
        assert len(hits) == 1, name
        assert int(hits[0]["private_segment_fixed_size"]) == 0, name
        assert int(hits[0]["group_segment_fixed_size"]) == lds, name
        m = re.search(r"<_Z\d+" + name + r"[^>]*>:\n(.*?)s_endpgm", dis, re.S)
        assert m, name
        body = m.group(1)
        assert "s_swappc" not in body and "v_sin" not in body and "v_cos" not in body and "scratch_" not in body, name
    assert "v_div_scale_f64" in re.search(r"<_Z\d+k_sim3_hypotheses[^>]*>:\n(.*?)s_endpgm", dis, re.S).group(1)


# ----------------------------------------------------------------------------------------------- sanitizers
def test_host_unit_clean_under_asan_ubsan(tmp_path):
    """csrc/orbx_sim3.cpp (validation, packing, the host path, the cursor; HIP-free) built with g++ -fsanitize=address,undefined
    together with tests/san_sim3.cpp: sizes around the mask words, every rejection, degenerate and non-finite input"""
    exe = str(tmp_path / "san_sim3")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_sim3.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_sim3.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr
