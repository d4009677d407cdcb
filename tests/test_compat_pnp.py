"""compat/PnPsolver.h (the drop-in for include/PnPsolver.h + src/PnPsolver.cc) compiled against the stand-ins of
tests/compat_pnp/ and the cv::Mat of tests/compat_runtime/, linked against liborbx.so and run: the constructor's filters and the
mvKeyPointIndices mapping (a bad MapPoint and a null slot included), SetRansacParameters, the draws, Prepare (one batch call for
all solvers) and a solver that runs alone, every iterate return, vbInliers in the slots of vpMapPointMatches, and the -2 / append
path (iterate(5) on a solver whose list is exhausted draws one more set at a time) -- against tests/pnp_model.py for the same
draws, bit for bit.  On a host-only handle here; on the device under the gpu marker."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pnp_model as pm
import pnp_scenes as ps
from orb_slam2_detailed_comments_amd import ORBextractor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "lib")
F = np.float32
DRAW_CAP = 200
RELOC = (0.99, 10, 300, 0.5)          # Relocalization's SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)


@pytest.fixture(scope="module")
def harness(built_lib, tmp_path_factory):
    assert shutil.which("g++")
    out = str(tmp_path_factory.mktemp("compat_pnp") / "harness.so")
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "tests", "compat_pnp"),
           "-I" + os.path.join(ROOT, "tests", "compat_runtime"), "-I" + os.path.join(ROOT, "compat"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "compat_pnp", "harness.cpp"), "-L" + LIBDIR, "-lorbx", "-Wl,-rpath," + LIBDIR, "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]
    L = C.CDLL(out)
    L.cp_error.restype = C.c_char_p
    L.cp_run.restype = C.c_int
    vp, i32 = C.c_void_p, C.c_int
    L.cp_run.argtypes = [vp, i32, i32] + [vp] * 5 + [C.c_double, i32, i32, C.c_float, C.c_uint64, i32, i32] + [vp] * 12 + [i32, vp, vp]
    return L


def level_sigma2():
    out, s = [], F(1)
    for _ in range(8):
        out.append(s * s)
        s = s * F(1.2)
    return np.array(out, F)


def scenario(seed, K=4, nslots=60):
    """one frame, K candidate match vectors: world points that project onto the frame's keypoints under each candidate's pose,
    a quarter of them wrong, with slots the constructor has to drop (NULL, bad) and one candidate with too few matches"""
    rng = np.random.default_rng(seed)
    cam = np.array(ps.CAMERA, F)
    kp = np.stack([rng.uniform(20, 620, nslots), rng.uniform(20, 460, nslots)], 1).astype(F)
    sc = dict(K=K, nslots=nslots, camera=cam, kp=kp, oct=rng.integers(0, 8, nslots).astype(np.int32),
              state=np.zeros((K, nslots), np.uint8), pos=np.zeros((K, nslots, 3), F))
    for k in range(K):
        T = np.eye(4)
        T[:3, :3] = ps.rotation(rng, 0.5)
        T[:3, 3] = rng.uniform(-1, 1, 3)
        z = rng.uniform(2, 20, nslots)
        Xc = np.stack([(kp[:, 0] - cam[2]) / cam[0] * z, (kp[:, 1] - cam[3]) / cam[1] * z, z], 1)
        wrong = rng.permutation(nslots)[:nslots // 4]
        Xc[wrong] += rng.uniform(1.0, 3.0, (len(wrong), 3)) * rng.choice([-1, 1], (len(wrong), 3))
        sc["pos"][k] = ((Xc - T[:3, 3]) @ T[:3, :3]).astype(F)
        st = sc["state"][k]
        drop = rng.choice(nslots, 9, replace=False)
        st[drop[:6]] = 1                                       # a null slot
        st[drop[6:]] = 2                                       # a bad MapPoint
        if k == K - 1:
            st[7:] = 1                                         # at most 7 correspondences: fewer than min_inliers
    return sc


def expected_problems(sc, params):
    probability, min_inliers, max_iterations, epsilon = params
    sig = level_sigma2()
    probs = []
    for k in range(sc["K"]):
        keep = np.nonzero(sc["state"][k] == 0)[0]
        mi, it = pm.set_ransac_parameters(len(keep), probability, min_inliers, max_iterations, 4, epsilon)
        probs.append(dict(p3dw=sc["pos"][k][keep], p2d=sc["kp"][keep], max_err=pm.max_error(sig[sc["oct"][keep]]),
                          camera=tuple(float(c) for c in sc["camera"]), min_inliers=mi, iterations=it, indices=keep, cache={}))
    return probs


def run(L, handle, sc, calls, prepare, params=RELOC, seed=12345):
    K, ns, nc = sc["K"], sc["nslots"], len(calls)
    ck = np.array([c[0] for c in calls], np.int32)
    cn = np.array([c[1] for c in calls], np.int32)
    out = dict(ret=np.full(nc, -9, np.int32), no_more=np.full(nc, -9, np.int32), nin=np.full(nc, -9, np.int32), T=np.zeros((nc, 16), F),
               inl=np.full((nc, ns), 9, np.uint8), inl_size=np.full(nc, -9, np.int32), n=np.zeros(K, np.int32),
               mi=np.zeros(K, np.int32), its=np.zeros(K, np.int32), kpi=np.full((K, ns), -1, np.int32),
               draws=np.full((K, DRAW_CAP * 4), -1, np.int32), ndraws=np.zeros(K, np.int32))
    ins = [np.ascontiguousarray(sc[k]) for k in ("state", "pos", "kp", "oct", "camera")]
    P = lambda a: a.ctypes.data_as(C.c_void_p)                 # noqa: E731
    rc = L.cp_run(handle, K, ns, *[P(a) for a in ins], params[0], params[1], params[2], params[3], seed, int(prepare), nc, P(ck), P(cn),
                  *[P(out[k]) for k in ("ret", "no_more", "nin", "T", "inl", "inl_size", "n", "mi", "its", "kpi")], DRAW_CAP,
                  P(out["draws"]), P(out["ndraws"]))
    assert rc == 0, L.cp_error().decode()
    return out


def check(L, handle, sc, calls, prepare, params=RELOC, seed=12345):
    got = run(L, handle, sc, calls, prepare, params, seed)
    probs = expected_problems(sc, params)
    assert [len(p["indices"]) for p in probs] == got["n"].tolist()
    assert [p["min_inliers"] for p in probs] == got["mi"].tolist() and [p["iterations"] for p in probs] == got["its"].tolist()
    for k, p in enumerate(probs):                              # mvKeyPointIndices: the kept slots in slot order
        assert np.array_equal(got["kpi"][k][:len(p["indices"])], p["indices"]), k
    rng = pm.Lcg(seed)
    solvers = {}

    def prepare_solver(k):                                     # the draws of a preparation: mRansacMaxIts sets, none when N < min
        p = probs[k]
        n = len(p["indices"])
        p["sets"] = rng.draw(n, p["iterations"]) if n >= p["min_inliers"] else np.zeros((0, 4), np.int32)
        solvers[k] = pm.Solver(p, pm.Own, p["cache"])

    if prepare:
        for k in range(sc["K"]):
            prepare_solver(k)
    returned = appended = 0
    for c, (k, nit) in enumerate(calls):
        if k not in solvers:
            prepare_solver(k)                                  # a solver that was not prepared prepares itself
        while True:
            m = solvers[k].iterate(nit)
            if m is not None:
                break
            solvers[k].append(rng.draw(len(probs[k]["indices"]), 1))          # the -2 path: one more set, then the call again
            appended += 1
        T, no_more, inl, nin = m
        assert got["ret"][c] == (T is not None) and got["no_more"][c] == no_more and got["nin"][c] == nin, (c, k)
        if T is None:
            assert got["inl_size"][c] == 0, (c, k)             # vbInliers stays cleared
            continue
        returned += 1
        slots = np.zeros(sc["nslots"], np.uint8)
        slots[probs[k]["indices"][inl]] = 1                    # vbInliers[mvKeyPointIndices[i]]
        assert got["inl_size"][c] == sc["nslots"] and np.array_equal(got["inl"][c], slots), (c, k)
        assert np.array_equal(ps.bits(got["T"][c]), ps.bits(T.reshape(-1))), (c, k)
    for k, sv in solvers.items():                              # every draw the shim made, the appended ones included
        want = np.array(sv.sets, np.int32).reshape(-1)
        assert got["ndraws"][k] == len(sv.sets) and np.array_equal(got["draws"][k][:len(want)], want), k
    return got, returned, appended


def both_ways(L, handle):
    sc = scenario(1)
    calls = [(k, 5) for _ in range(3) for k in range(4)]
    got, returned, appended = check(L, handle, sc, calls, prepare=True)
    assert returned >= 3 and got["no_more"][3] == 1 and got["n"][3] <= 7         # the short candidate is "no more" at its first call
    assert sc["state"][0].tolist().count(1) == 6 and sc["state"][0].tolist().count(2) == 3
    # the same solvers, each running alone from its first iterate: solver 2 is called first, so it draws first
    got2, returned2, _ = check(L, handle, sc, [(2, 5), (0, 5)] + calls, prepare=False)
    assert returned2 >= 3 and not np.array_equal(got["draws"], got2["draws"])     # other draws: another order of RandomInt calls
    # iterated again and again after every answer was rejected: past mRansacMaxIts every call draws, appends and goes on
    _, returned3, appended3 = check(L, handle, scenario(2, K=2), [(0, 5)] * 30 + [(1, 300)], prepare=True)
    assert appended3 > 0 and returned3 > 5


def test_shim_equals_the_model_on_a_host_only_handle(harness):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    try:
        both_ways(harness, ex.handle)
    finally:
        ex.close()


@pytest.mark.gpu
def test_shim_equals_the_model_on_the_device(harness):
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=True)
    ex = ORBextractor(1000, 1.2, 8, 20, 7)
    try:
        both_ways(harness, ex.handle)
    finally:
        ex.close()
        faulthandler.cancel_dump_traceback_later()
