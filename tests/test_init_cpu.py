"""Initializer H / F RANSAC (orbx_init_ransac_batch_create and its accessors), the part that needs no GPU: the library's host path
through the C ABI against tests/init_model.py, bit for bit as uint32 -- T1 and T2, every hypothesis matrix and inverse, every
score, every mask word, the best iterations, RH, the model -- in both fp_modes; planted scenes with a known model; validation
before any work; the distance of the library's null vector from LAPACK's; the HIP-free unit under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/san_init.cpp, a stand-alone program); no scratch in the two kernels and the LDS the header's
constants give.

The contract is device = host path = model.  Parity with an OpenCV build is not pinned.

Accuracy.  The same A matrices (float32, built by the model from the normalised draws of the planted scenes) go through
numpy.linalg.svd in float64; the library's null vector, scaled to unit norm in float64 and sign-aligned, is compared entry by
entry.  All 200 H systems of every planted scene take part; the F systems of the two general 3-D scenes do (on a plane or under
a pure rotation the 8 x 9 system of F has a null space of more than one dimension and no vector to compare).  The figures are
measured on the CPU and recorded in DESIGN.md F14; the test asserts four times each, the scenes are fixed, so the margin only
absorbs another libm or LAPACK."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import init_model as im
import init_scenes as sc
from orb_slam2_detailed_comments_amd import InitializerRansac, ORBextractor, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NULL_H_MEASURED, NULL_F_MEASURED = 6.921e-7, 6.334e-5          # largest |x - x_lapack| over the H systems, over the F systems


@pytest.fixture(scope="module", params=[_capi.FP_GCC_FMA, _capi.FP_STRICT], ids=["fma", "strict"])
def host(request, built_lib):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2, fp_mode=request.param)
    yield ex
    ex.close()


def run(host, problems, what=""):
    rb = InitializerRansac(host, problems)
    try:
        sc.assert_batch_equals_model(rb, problems, what)
        return [rb.result(k) for k in range(len(problems))]
    finally:
        rb.close()


# ----------------------------------------------------------------------------------------------- planted scenes
def test_planted_scenes_equal_the_model_and_choose_the_planted_model(host):
    problems = list(sc.planted_scenes())
    assert [p["kind"] for p in problems] == ["plane", "general", "rotation", "general"]
    for p in problems:                                          # planted outliers are displaced by 20 px or more
        assert (~p["planted_inlier"]).sum() >= 20
    res = run(host, problems, "planted")
    for p, r in zip(problems, res):
        want = im.FUND if p["kind"] == "general" else im.H
        assert r["model"] == want, p["kind"]
        mask = r["inliersH"] if want == im.H else r["inliersF"]
        assert (mask == p["planted_inlier"]).all(), p["kind"]   # every planted inlier, no planted outlier
        assert (r["RH"] > 0.40) == (want == im.H)


def test_normalization_runs_over_all_keypoints_not_over_the_matched_ones(host):
    p = sc.planted_scenes()[3]
    assert len(p["keys1"]) - len(p["matches"]) == 300 and len(p["keys2"]) - len(p["matches"]) == 200
    rb = InitializerRansac(host, [p])
    T1, T2 = rb.normalization(0)
    rb.close()
    for T, keys, col in ((T1, p["keys1"], 0), (T2, p["keys2"], 1)):
        own, _ = im.normalize(keys)
        matched, _ = im.normalize(keys[p["matches"][:, col]])
        assert np.array_equal(sc.bits(T), sc.bits(own))
        assert abs(matched[0, 2] - own[0, 2]) > 0.5 and matched[0, 0] != own[0, 0] and matched[1, 1] != own[1, 1]   # the cluster moves mean and scale


def test_degenerate_sets_are_not_finite_and_lose(host):
    p = sc.degenerate()
    r = run(host, [p], "degenerate")[0]
    mo = sc.model_of(p)
    h = mo["per"][im.H]
    assert h["bad"][0] and np.isnan(h["scores"][0])             # eight coinciding points: H is singular, its inverse is not finite
    assert (sc.bits(h["Minv"][0]) & 0x7f800000 == 0x7f800000).all()
    assert h["masks"][0].all()                                  # a NaN chi-square leaves bIn alone, as in the source
    for name, model in (("H", im.H), ("F", im.FUND)):
        per = mo["per"][model]
        assert r["it" + name] >= 0 and not per["bad"][r["it" + name]] and np.isfinite(per["scores"][r["it" + name]])
        assert not (per["bad"] & (per["scores"] > 0)).any()     # no hypothesis that is not finite scores at all
    assert np.isfinite(mo["per"][im.FUND]["M"][1]).all()        # collinear points: a finite matrix like any other


def test_nothing_scores_gives_none(host):
    probs = list(sc.none_scenes())
    res = run(host, probs, "none")
    for r in res:
        assert r["model"] == im.NONE and r["itH"] == r["itF"] == -1 and r["SH"] == 0 and r["SF"] == 0
        assert sc.bits(r["RH"]) == 0x7fc00000 and not r["H21"].any() and not r["F21"].any()
        assert not r["inliersH"].any() and not r["inliersF"].any()
    mo = sc.model_of(probs[1])                                  # NaN keypoints: every score is the canonical NaN, every mask all-true
    assert (sc.bits(mo["per"][im.H]["scores"]) == 0x7fc00000).all() and mo["per"][im.FUND]["masks"].all()
    assert (sc.model_of(probs[0])["per"][im.H]["scores"] == 0).all()


# ----------------------------------------------------------------------------------------------- sizes, batches
def test_size_list_and_mixed_call(host):
    run(host, list(sc.size_problems()), "sizes")
    mixed = sc.mixed_call()
    assert sum(not sc.launches(p) for p in mixed) == 2
    run(host, mixed, "mixed")
    for k, p in enumerate(mixed):                              # batch = single calls
        run(host, [p], f"single {k}")
    rb = InitializerRansac(host, [])
    assert len(rb) == 0
    rb.close()


def test_models_not_requested_and_the_choice_between_them(host):
    p = sc.planted_scenes()[0]
    both, only_h, only_f = run(host, [p, sc.variant(p, models=im.H), sc.variant(p, models=im.FUND)], "models")
    assert only_h["model"] == im.H and only_h["RH"] == 1 and sc.bits(only_h["SH"]) == sc.bits(both["SH"]) and only_h["itF"] == -1
    assert only_f["model"] == im.FUND and only_f["RH"] == 0 and sc.bits(only_f["SF"]) == sc.bits(both["SF"]) and only_f["itH"] == -1
    assert not only_h["inliersF"].any() and not only_f["inliersH"].any()


# ----------------------------------------------------------------------------------------------- validation
def test_validation_before_any_work(host):
    L, B, OK = _capi.lib(), _capi.BAD_ARGUMENT, _capi.OK
    p = sc.make(90, 12, "plane", iterations=4, extra1=3, extra2=5)
    arr = (_capi.InitProblem * 2)()
    keep = [np.ascontiguousarray(p[k]) for k in ("keys1", "keys2")] + [p["matches"].copy(), p["sets"].copy()]

    def fill():
        for a in arr:
            a.n1, a.n2, a.n = 15, 17, 12
            a.keys1, a.keys2, a.matches, a.sets = (v.ctypes.data for v in keep)
            a.sigma, a.iterations, a.models = 1.0, 4, 3

    def call(n=2, pr=arr, h=host.handle, out=True):
        b = C.c_void_p()
        st = L.orbx_init_ransac_batch_create(h, n, C.cast(pr, C.c_void_p) if pr is not None else None, C.byref(b) if out else None)
        if st == OK:
            L.orbx_init_batch_destroy(b)
        return st

    fill()
    assert call() == OK
    assert call(n=-1) == B and call(pr=None) == B and call(h=None) == B and call(out=False) == B
    assert call(n=0, pr=None) == OK
    for field, value in (("n", -1), ("n1", -1), ("n2", -1), ("iterations", 0), ("iterations", -3), ("keys1", None), ("keys2", None),
                         ("matches", None), ("sets", None), ("sigma", 0.0), ("sigma", -1.0), ("sigma", float("inf")),
                         ("sigma", float("nan")), ("models", 4), ("models", -1)):
        fill()
        setattr(arr[1], field, value)
        assert call() == B, (field, value)
    for col, bad in ((0, 15), (0, -1), (1, 17), (1, -1)):       # a match index outside its frame
        fill()
        keep[2][5, col] = bad
        assert call() == B, (col, bad)
        keep[2][:] = p["matches"]
    for bad in (12, -1):                                        # a set index outside [0, n)
        fill()
        keep[3][2, 1] = bad
        assert call() == B, bad
        keep[3][:] = p["sets"]
    fill()
    keep[3][3, 6] = keep[3][3, 0]                              # an index repeated within its set: the reference's draw cannot repeat
    assert call() == B
    assert b"repeated" in L.orbx_last_error()
    keep[3][:] = p["sets"]
    fill()
    arr[1].n, arr[1].matches, arr[1].sets = 7, keep[2].ctypes.data, None    # n < 8: the sets are not read
    assert call() == OK
    arr[1].n, arr[1].n1, arr[1].n2, arr[1].keys1, arr[1].keys2, arr[1].matches = 0, 0, 0, None, None, None
    assert call() == OK
    rb = InitializerRansac(host, [p])
    assert L.orbx_init_batch_result(rb._b, 1, *[None] * 10) == B and L.orbx_init_batch_result(rb._b, -1, *[None] * 10) == B
    assert L.orbx_init_batch_result(None, 0, *[None] * 10) == B and L.orbx_init_batch_result(rb._b, 0, *[None] * 10) == OK
    assert L.orbx_init_batch_hypothesis(rb._b, 0, im.H, 4, None, None, None, None) == B
    assert L.orbx_init_batch_hypothesis(rb._b, 0, im.H, 3, None, None, None, None) == OK
    assert L.orbx_init_batch_hypothesis(rb._b, 0, 3, 0, None, None, None, None) == B
    assert L.orbx_init_batch_scores(rb._b, 0, 0, None, None) == B and L.orbx_init_batch_scores(rb._b, 0, im.FUND, None, None) == OK
    assert L.orbx_init_batch_normalization(rb._b, 2, None, None) == B and L.orbx_init_batch_normalization(rb._b, 0, None, None) == OK
    rb.close()


# ----------------------------------------------------------------------------------------------- accuracy
def test_distance_of_the_null_vector_from_lapack(built_lib):
    worst = {"H": 0.0, "F": 0.0}
    used = {"H": 0, "F": 0}
    for p in sc.planted_scenes():
        k1, k2, m = p["keys1"], p["keys2"], p["matches"]
        _, (mx1, my1, sx1, sy1) = im.normalize(k1)
        _, (mx2, my2, sx2, sy2) = im.normalize(k2)
        a, b = k1[m[:, 0]], k2[m[:, 1]]
        pn = np.stack([(a[:, 0] - mx1) * sx1, (a[:, 1] - my1) * sy1, (b[:, 0] - mx2) * sx2, (b[:, 1] - my2) * sy2], axis=1).astype(F)
        for name, is_h in (("H", True), ("F", False)):
            if not is_h and p["kind"] != "general":
                continue
            A = im.build_A(pn[p["sets"]], is_h)
            x = im.null_vector(A).astype(np.float64)
            x /= np.linalg.norm(x, axis=1, keepdims=True)
            ref = np.linalg.svd(A.astype(np.float64), full_matrices=True)[2][:, 8, :]
            sign = np.sign((x * ref).sum(axis=1))
            worst[name] = max(worst[name], float(np.abs(x - sign[:, None] * ref).max()))
            used[name] += len(A)
    for name in worst:
        print(f"{name}: {used[name]} systems; largest |x - x_lapack| = {worst[name]:.3e}")
    assert used == {"H": 800, "F": 400}
    assert worst["H"] <= 4 * NULL_H_MEASURED and worst["F"] <= 4 * NULL_F_MEASURED


# ----------------------------------------------------------------------------------------------- sanitizers
def test_host_unit_clean_under_asan_ubsan(tmp_path):
    """csrc/orbx_init.cpp (validation, Normalize, packing, the host path, the result object; HIP-free) built with g++
    -fsanitize=address,undefined together with tests/san_init.cpp, a stand-alone program: sizes around the mask words, every
    rejection, problems that launch nothing, degenerate and non-finite input"""
    exe = str(tmp_path / "san_init")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_init.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_init.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr


# ----------------------------------------------------------------------------------------------- the kernels in the code object
def test_kernels_have_no_scratch_and_fit_the_lds(built_lib):
    from test_pipeline_room import _kernel_metadata
    meta = _kernel_metadata(built_lib)
    ws_floats = 16 * 9 + 9 * 9 + 8 * 4                          # A | V | the eight drawn matches: ORBX_INIT_WS_FLOATS
    for name, lds in (("k_init_hypotheses", ws_floats * sc.HYP_LANES * 4), ("k_init_scores", 4 * sc.CHUNK * 4)):
        hits = [v for k, v in meta.items() if name in k]
        assert len(hits) == 1, name
        assert int(hits[0]["private_segment_fixed_size"]) == 0, name
        assert int(hits[0]["group_segment_fixed_size"]) == lds and lds <= 160 * 1024, name
