"""ReconstructH / ReconstructF with DecomposeE, CheckRT and Triangulate (orbx_init_reconstruct_batch_create and its accessors), the
part that needs no GPU: the library's host path through the C ABI against tests/recon_model.py, bit for bit as uint32 -- every R,
t, n, count, cosine, parallax, status byte, point, the chosen hypothesis and ok -- in both fp_modes; scenes that show each edge of
the source ON THE MODEL ALONE; validation before any work; the properties of the 3 x 3 SVD; the distance of the chosen motion
from a float64 restatement and from the planted motion; the HIP-free unit under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/san_recon.cpp, a stand-alone program); no scratch in the new kernels and the LDS the header's constants give.

The contract is device = host path = model.  Parity with an OpenCV build is not pinned.

Accuracy.  For every scene whose reconstruction succeeds the same float32 matrix goes through numpy.linalg.svd in float64 and the
source's formulas in float64 (the four poses of DecomposeE, the eight of ReconstructH); the library's R21 is compared entry by
entry with the nearest of those poses and t21 by the angle between the directions, and both with the planted motion.  The
figures are measured on the CPU and recorded in DESIGN.md F15; the test asserts four times each, the scenes are fixed, so the
margin only absorbs another libm or LAPACK."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recon_model as rm
import recon_scenes as sc
from orb_slam2_detailed_comments_amd import InitializerReconstruct, ORBextractor, _capi
from orb_slam2_detailed_comments_amd.initializer import scatter_matches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
# largest |R21 - R| (entry) and largest angle (degrees) between t21 and t: against the float64 restatement, against the planted motion
R_F64_MEASURED, T_F64_MEASURED, R_PLANTED_MEASURED, T_PLANTED_MEASURED = 5.745e-7, 9.440e-5, 5.861e-7, 7.575e-5


@pytest.fixture(scope="module", params=[_capi.FP_GCC_FMA, _capi.FP_STRICT], ids=["fma", "strict"])
def host(request, built_lib):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2, fp_mode=request.param)
    yield ex
    ex.close()


def run(host, problems, what=""):
    rc = InitializerReconstruct(host, problems)
    try:
        sc.assert_batch_equals_model(rc, problems, what)
        return [rc.result(k) for k in range(len(problems))]
    finally:
        rc.close()


# ----------------------------------------------------------------------------------------------- the scenes, on the model alone
def test_the_model_alone_shows_every_case():
    c = sc.cases()
    mo = {k: sc.model_of(p) for k, p in c.items()}
    good = {k: [h["nGood"] for h in m["hyp"]] for k, m in mo.items()}
    assert mo["plane_h"]["ok"] and c["plane_h"]["model"] == rm.H and sorted(good["plane_h"])[-2] > 0      # accepted against a runner-up
    assert mo["general_f"]["ok"] and c["general_f"]["model"] == rm.FUND
    r = mo["rotation_h"]                                         # d1 / d2 < 1.00001: no hypothesis is evaluated
    assert not r["ok"] and r["chosen"] == -1 and not any(h["valid"] for h in r["hyp"]) and r["N"] == 80
    assert np.float64(r["svd"]["w"][0] / r["svd"]["w"][1]) < 1.00001
    lp, g = mo["low_parallax_f"], good["low_parallax_f"]        # every count test passes, only the parallax does not
    assert not lp["ok"] and max(g) >= max(int(0.9 * lp["N"]), 50) and sum(x > 0.7 * max(g) for x in g) == 1
    assert 0 < lp["hyp"][lp["chosen"]]["parallax"] <= 1.0
    assert rm.solve(sc.variant(c["low_parallax_f"], min_parallax=0.5))["ok"]
    g = good["tie_f"]                                            # a later hypothesis ties maxGood; the first is the candidate
    assert g.count(max(g)) >= 2 and mo["tie_f"]["chosen"] == g.index(max(g)) and not mo["tie_f"]["ok"]
    for k in sc.WINNER_COUNTS:
        assert max(good[f"winner_{k}"]) == k, k
    assert [mo[f"winner_{k}"]["ok"] for k in sc.WINNER_COUNTS] == [False, False, True, True, True, True]   # ReconstructF: maxGood < nMinGood fails, 50 does not
    b = mo["behind_f"]                                           # counted, not flagged, behind the camera
    assert b["status"][0] == 2 and b["points"][0, 2] < 0 and b["ok"]
    nf, p = mo["nonfinite_repeated_f"], c["nonfinite_repeated_f"]
    assert nf["status"][40] == 1 and nf["status"][3] == 3 and nf["status"][5] == 3 and nf["status"][41] == 3 and nf["ok"]
    assert p["matches"][40, 0] == p["matches"][3, 0] and p["matches"][41, 0] == p["matches"][5, 0]
    P3, tri = scatter_matches(nf, p["matches"], len(p["keys1"]))
    assert not tri[p["matches"][3, 0]] and tri[p["matches"][5, 0]] and tri.sum() == 57      # 59 flagged matches, one reset, one pair repeated
    for k in ("all_false", "n0"):
        assert not mo[k]["ok"] and mo[k]["N"] == 0 and mo[k]["chosen"] == -1 and not any(h["nGood"] for h in mo[k]["hyp"])
    assert mo["plane_as_f"]["ok"] and mo["general_as_h"]["ok"]


# ----------------------------------------------------------------------------------------------- host path = model
def test_every_case_equals_the_model_and_the_first_four_come_out_as_listed(host):
    c = sc.cases()
    res = dict(zip(c, run(host, list(c.values()), "cases")))
    assert res["plane_h"]["ok"] and res["general_f"]["ok"]
    assert not res["rotation_h"]["ok"] and res["rotation_h"]["chosen"] == -1 and not res["rotation_h"]["status"].any()
    assert not res["low_parallax_f"]["ok"] and not res["low_parallax_f"]["R21"].any() and res["low_parallax_f"]["status"].any()
    for k, p in c.items():                                       # the planted inliers of an accepted scene are triangulated
        if res[k]["ok"] and k not in ("behind_f", "nonfinite_repeated_f"):
            assert ((res[k]["status"] == 3) == p["inliers"]).all(), k


def test_size_list_mixed_call_and_single_calls(host):
    run(host, list(sc.size_problems()), "sizes")
    mixed = sc.mixed_call()
    assert sum(sc.model_of(p)["N"] == 0 for p in mixed) == 2 and {p["model"] for p in mixed} == {rm.H, rm.FUND}
    run(host, mixed, "mixed")
    for k, p in enumerate(mixed):                              # batch = single calls
        run(host, [p], f"single {k}")
    rc = InitializerReconstruct(host, [])
    assert len(rc) == 0
    rc.close()


# ----------------------------------------------------------------------------------------------- validation
def test_validation_before_any_work(host):
    L, B, OK = _capi.lib(), _capi.BAD_ARGUMENT, _capi.OK
    p = sc.cases()["winner_51"]
    arr = (_capi.ReconProblem * 2)()
    keep = [np.ascontiguousarray(p["keys1"]), np.ascontiguousarray(p["keys2"]), p["matches"].copy(), p["inliers"].astype(np.uint8)]
    n1, n2, n = len(keep[0]), len(keep[1]), len(keep[2])

    def fill():
        for a in arr:
            a.n1, a.n2, a.n = n1, n2, n
            a.keys1, a.keys2, a.matches, a.inliers = (v.ctypes.data for v in keep)
            a.model, a.sigma, a.min_parallax, a.min_triangulated = rm.FUND, 1.0, 1.0, 50
            a.M[:] = [float(v) for v in p["M"].reshape(9)]
            a.K[:] = sc.K4

    def call(nprob=2, pr=arr, h=host.handle, out=True):
        b = C.c_void_p()
        st = L.orbx_init_reconstruct_batch_create(h, nprob, C.cast(pr, C.c_void_p) if pr is not None else None, C.byref(b) if out else None)
        if st == OK:
            L.orbx_recon_batch_destroy(b)
        return st

    fill()
    assert call() == OK
    assert call(nprob=-1) == B and call(pr=None) == B and call(h=None) == B and call(out=False) == B
    assert call(nprob=0, pr=None) == OK
    inf, nan = float("inf"), float("nan")
    for field, value in (("n", -1), ("n1", -1), ("n2", -1), ("keys1", None), ("keys2", None), ("matches", None), ("inliers", None),
                         ("model", 0), ("model", 3), ("model", -1), ("sigma", 0.0), ("sigma", -1.0), ("sigma", inf), ("sigma", nan),
                         ("min_parallax", nan)):
        fill()
        setattr(arr[1], field, value)
        assert call() == B, (field, value)
    for i, value in ((0, 0.0), (0, -1.0), (0, inf), (0, nan), (1, 0.0), (1, nan), (2, nan), (2, inf), (3, nan), (3, -inf)):
        fill()
        arr[1].K[i] = value
        assert call() == B, (i, value)
    assert b"intrinsic" in L.orbx_last_error()
    for col, bad in ((0, n1), (0, -1), (1, n2), (1, -1)):       # a match index outside its frame
        fill()
        keep[2][5, col] = bad
        assert call() == B, (col, bad)
        keep[2][:] = p["matches"]
    fill()
    arr[1].n, arr[1].n1, arr[1].n2, arr[1].keys1, arr[1].keys2, arr[1].matches, arr[1].inliers = 0, 0, 0, None, None, None, None
    assert call() == OK
    rc = InitializerReconstruct(host, [p])
    assert L.orbx_recon_batch_result(rc._b, 1, *[None] * 7) == B and L.orbx_recon_batch_result(rc._b, -1, *[None] * 7) == B
    assert L.orbx_recon_batch_result(None, 0, *[None] * 7) == B and L.orbx_recon_batch_result(rc._b, 0, *[None] * 7) == OK
    assert L.orbx_recon_batch_hypothesis(rc._b, 0, 4, *[None] * 7) == B and L.orbx_recon_batch_hypothesis(rc._b, 0, 3, *[None] * 7) == OK
    assert L.orbx_recon_batch_hypothesis(rc._b, 0, -1, *[None] * 7) == B
    rc.close()


# ----------------------------------------------------------------------------------------------- the 3 x 3 SVD
def test_properties_of_the_3x3_svd_on_the_matrices_of_the_scenes():
    """the SVD is not exported; the host path's R, t and n are functions of it and equal the model's bit for bit, so the
    properties are checked on the model's U, w, Vt of every E and A the scenes give"""
    seen = 0
    for name, p in list(sc.cases().items()) + [(f"size {i}", q) for i, q in enumerate(sc.size_problems())]:
        s = sc.model_of(p)["svd"]
        if s is None:
            continue
        U, w, Vt, M = (np.asarray(s[k], np.float64) for k in ("U", "w", "Vt", "M"))
        scale = w[0]
        assert np.abs(U.T @ U - np.eye(3)).max() < 1e-5, name
        assert np.abs(Vt @ Vt.T - np.eye(3)).max() < 1e-5, name
        assert np.abs(U @ np.diag(w) @ Vt - M).max() < 1e-5 * scale, name
        assert w[0] >= w[1] >= w[2] >= 0, name
        ref = np.linalg.svd(M, compute_uv=False)
        assert np.abs(w - ref).max() < 1e-5 * scale, name
        seen += 1
    assert seen >= 25


# ----------------------------------------------------------------------------------------------- accuracy
def _poses_f64(p):
    K = sc.K
    M = np.asarray(p["M"], np.float64)
    if p["model"] == rm.FUND:
        U, _, Vt = np.linalg.svd(K.T @ M @ K)
        W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
        out = []
        for t in (U[:, 2], -U[:, 2]):
            for R in (U @ W @ Vt, U @ W.T @ Vt):
                out.append((R if np.linalg.det(R) > 0 else -R, t))
        return out
    U, (d1, d2, d3), Vt = np.linalg.svd(np.linalg.inv(K) @ M @ K)
    s = np.linalg.det(U) * np.linalg.det(Vt)
    aux1, aux3 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    root = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
    st, ct = root / ((d1 + d3) * d2), (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    sp, cp = root / ((d1 - d3) * d2), (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    out = []
    for i, (e1, e3) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))):
        sg = 1 if i in (0, 3) else -1
        Rp = np.array([[ct, 0, -sg * st], [0, 1, 0], [sg * st, 0, ct]])
        tp = np.array([e1 * aux1, 0, -e3 * aux3]) * (d1 - d3)
        out.append((s * U @ Rp @ Vt, U @ tp / np.linalg.norm(U @ tp)))
        Rp = np.array([[cp, 0, sg * sp], [0, -1, 0], [sg * sp, 0, -cp]])
        tp = np.array([e1 * aux1, 0, e3 * aux3]) * (d1 + d3)
        out.append((s * U @ Rp @ Vt, U @ tp / np.linalg.norm(U @ tp)))
    return out


def _angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.degrees(np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1, 1))))


def test_distance_of_the_chosen_motion_from_float64_and_from_the_planted_motion(host):
    worst = dict(R64=0.0, t64=0.0, Rp=0.0, tp=0.0)
    used = 0
    for name, p in sc.cases().items():
        r = run(host, [p], name)[0]
        if not r["ok"]:
            continue
        R21, t21 = r["R21"].astype(np.float64), r["t21"].astype(np.float64)
        R, t = min(_poses_f64(p), key=lambda c: np.abs(R21 - c[0]).max() + np.radians(_angle(t21, c[1])))
        worst["R64"], worst["t64"] = max(worst["R64"], float(np.abs(R21 - R).max())), max(worst["t64"], _angle(t21, t))
        worst["Rp"] = max(worst["Rp"], float(np.abs(R21 - p["R_true"]).max()))
        worst["tp"] = max(worst["tp"], _angle(t21, p["t_true"]))
        used += 1
    print(f"{used} accepted scenes; largest |R21 - R_f64| = {worst['R64']:.3e}, angle(t21, t_f64) = {worst['t64']:.3e} deg; "
          f"largest |R21 - R_planted| = {worst['Rp']:.3e}, angle(t21, t_planted) = {worst['tp']:.3e} deg")
    assert used == 10
    assert worst["R64"] <= 4 * R_F64_MEASURED and worst["t64"] <= 4 * T_F64_MEASURED
    assert worst["Rp"] <= 4 * R_PLANTED_MEASURED and worst["tp"] <= 4 * T_PLANTED_MEASURED


# ----------------------------------------------------------------------------------------------- sanitizers
def test_host_unit_clean_under_asan_ubsan(tmp_path):
    """csrc/orbx_recon.cpp (validation, packing, the host path, acos and the accept / reject arithmetic, the result object;
    HIP-free) built with g++ -fsanitize=address,undefined together with tests/san_recon.cpp, a stand-alone program: sizes around
    the ballot words, both models, every rejection, problems that launch nothing, non-finite input, a RANSAC batch continued"""
    exe = str(tmp_path / "san_recon")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_recon.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_recon.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr


# ----------------------------------------------------------------------------------------------- the kernels in the code object
def test_kernels_have_no_scratch_and_fit_the_lds(built_lib):
    from test_pipeline_room import _kernel_metadata
    meta = _kernel_metadata(built_lib)
    ws_floats, lanes = 9 + 9, 64                                 # the 3 x 3 matrix and its V: ORBX_RECON_WS_FLOATS, ORBX_RECON_LANES
    for name, lds in (("k_init_decompose", ws_floats * lanes * 4), ("k_init_check_rt", 0), ("k_init_pick", 0), ("k_init_select", 0)):
        hits = [v for k, v in meta.items() if name in k]
        assert len(hits) == 1, name
        assert int(hits[0]["private_segment_fixed_size"]) == 0, name
        assert int(hits[0]["group_segment_fixed_size"]) == lds and lds <= 160 * 1024, name


# ----------------------------------------------------------------------------------------------- the fused call, host path
def test_initialize_batch_on_the_host_path_equals_the_two_calls(host):
    import init_scenes as isc
    from orb_slam2_detailed_comments_amd import InitializerRansac, initialize_batch
    probs = sc.ransac_problems()
    cams = [sc.camera() for _ in probs]
    rb, rc = initialize_batch(host, probs, cams)
    rb2 = InitializerRansac(host, probs)
    try:
        isc.assert_batch_equals_model(rb, probs, "fused: RANSAC half")
        alone = [sc.from_ransac(p, rb2.result(k), cams[k]) for k, p in enumerate(probs)]
        sc.assert_batch_equals_model(rc, alone, "fused: reconstruction half")
        ran, rec = [rb.result(k) for k in range(len(probs))], [rc.result(k) for k in range(len(probs))]
        assert [r["model"] for r in ran][:5] == [rm.H, rm.FUND, rm.im.NONE, rm.H, rm.im.NONE]
        assert rec[1]["ok"] and not rec[2]["ok"] and not rec[3]["ok"] and not rec[4]["ok"] and rec[2]["N"] == 0
    finally:
        rb.close(), rc.close(), rb2.close()
    L, B = _capi.lib(), _capi.BAD_ARGUMENT
    arr = (_capi.InitProblem * 1)()
    cam = (_capi.InitCamera * 1)()
    cam[0].K[:] = sc.K4
    b1, b2 = C.c_void_p(), C.c_void_p()
    arr[0].sigma, arr[0].iterations, arr[0].models = 1.0, 1, 3   # no keypoints, no matches: valid, launches nothing
    assert L.orbx_initialize_batch_create(host.handle, 1, arr, cam, C.byref(b1), C.byref(b2)) == _capi.OK
    L.orbx_init_batch_destroy(b1), L.orbx_recon_batch_destroy(b2)
    assert L.orbx_initialize_batch_create(host.handle, 1, arr, None, C.byref(b1), C.byref(b2)) == B
    assert L.orbx_initialize_batch_create(host.handle, 1, arr, cam, None, C.byref(b2)) == B
    assert L.orbx_initialize_batch_create(host.handle, 1, arr, cam, C.byref(b1), None) == B
    for i, v in ((0, 0.0), (1, float("nan")), (2, float("inf"))):
        cam[0].K[:] = sc.K4
        cam[0].K[i] = v
        assert L.orbx_initialize_batch_create(host.handle, 1, arr, cam, C.byref(b1), C.byref(b2)) == B, (i, v)
    cam[0].K[:] = sc.K4
    arr[0].sigma = 0.0
    assert L.orbx_initialize_batch_create(host.handle, 1, arr, cam, C.byref(b1), C.byref(b2)) == B
