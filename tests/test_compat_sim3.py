"""compat/Sim3Solver.h (the drop-in for include/Sim3Solver.h + src/Sim3Solver.cc) compiled against the stand-ins of
tests/compat_sim3/ and the cv::Mat of tests/compat_runtime/, linked against liborbx.so and run: the constructor's filters and the
mvnIndices1 mapping, SetRansacParameters, the draws, Prepare (one batch call for all solvers) and a solver that runs alone, every
iterate return, vbInliers in the slots of vpMatched12, and GetEstimated* -- against tests/sim3_model.py for the same draws, bit
for bit.  On a host-only handle here; on the device under the gpu marker."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import sim3_model as sm
import sim3_scenes as ss
from orb_slam2_detailed_comments_amd import ORBextractor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "lib")
F = np.float32
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def harness(built_lib, tmp_path_factory):
    assert shutil.which("g++")
    out = str(tmp_path_factory.mktemp("compat_sim3") / "harness.so")
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "tests", "compat_sim3"),
           "-I" + os.path.join(ROOT, "tests", "compat_runtime"), "-I" + os.path.join(ROOT, "compat"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "compat_sim3", "harness.cpp"), "-L" + LIBDIR, "-lorbx", "-Wl,-rpath," + LIBDIR, "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]
    L = C.CDLL(out)
    L.cs_error.restype = C.c_char_p
    L.cs_run.restype = C.c_int
    vp, i32 = C.c_void_p, C.c_int
    L.cs_run.argtypes = [vp, i32, i32] + [vp] * 10 + [i32, C.c_double, i32, i32, C.c_uint64, i32, i32] + [vp] * 12
    return L


class Lcg:
    """tests/compat_sim3/Thirdparty/DBoW2/DUtils/Random.h"""

    def __init__(self, seed):
        self.s = seed

    def randint(self, lo, hi):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & MASK
        return lo + (self.s >> 33) % (hi - lo + 1)

    def draw(self, n, iterations):
        out = np.zeros((iterations, 3), np.int32)
        for i in range(iterations):
            avail = list(range(n))
            for c in range(3):
                r = self.randint(0, len(avail) - 1)
                out[i, c] = avail[r]
                avail[r] = avail[-1]
                avail.pop()
        return out


def camera_frame(T, X):
    """Rcw * Xw + tcw as the cv::Mat stand-in computes it: the row sum in double (k = 0, 1, 2), rounded once, then + t in float"""
    T = T.astype(np.float64)
    X64 = X.astype(np.float64)
    rows = [(((0.0 + T[r, 0] * X64[:, 0]) + T[r, 1] * X64[:, 1]) + T[r, 2] * X64[:, 2]).astype(F) + F(T[r, 3]) for r in range(3)]
    return np.stack(rows, axis=1).astype(F)


def level_sigma2():
    out, s = [], F(1)
    for _ in range(8):
        out.append(s * s)
        s = s * F(1.2)
    return np.array(out, F)


def scenario(seed, K=4, nslots=48):
    """K candidates against one current keyframe: planted Sim3 scenes in world coordinates under non-trivial poses, with slots
    that the constructor has to drop (no match, NULL, bad, not observed) and one candidate with too few correspondences"""
    rng = np.random.default_rng(seed)
    T1 = np.eye(4, dtype=F)
    T1[:3, :3] = ss.rotation(rng.normal(size=3), 0.2).astype(F)
    T1[:3, 3] = rng.uniform(-0.5, 0.5, 3)
    sc = dict(K=K, nslots=nslots, T1=T1, K1=ss.CAMERA1, T2=np.zeros((K, 4, 4), F), K2=np.zeros((K, 4), F),
              state1=np.zeros((K, nslots), np.uint8), state2=np.zeros((K, nslots), np.uint8), pos1=np.zeros((K, nslots, 3), F),
              pos2=np.zeros((K, nslots, 3), F), oct1=rng.integers(0, 8, (K, nslots)).astype(np.int32),
              oct2=rng.integers(0, 8, (K, nslots)).astype(np.int32))
    for k in range(K):
        p = ss.make(700 + 10 * seed + k, nslots, iterations=1, outlier_frac=0.25)
        T2 = np.eye(4, dtype=F)
        T2[:3, :3] = ss.rotation(rng.normal(size=3), 0.3).astype(F)
        T2[:3, 3] = rng.uniform(-0.5, 0.5, 3)
        sc["T2"][k], sc["K2"][k] = T2, ss.CAMERA2 * F(1 + 0.01 * k)
        # world positions whose camera-frame images are (about) the scene's x1c, x2c
        for T, x, key in ((T1, p["x1c"], "pos1"), (T2, p["x2c"], "pos2")):
            R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
            sc[key][k] = ((x.astype(np.float64) - t) @ R).astype(F)
        st1, st2 = sc["state1"][k], sc["state2"][k]
        drop = rng.choice(nslots, 12, replace=False)
        st2[drop[:4]] = 1                                      # vpMatched12[i] == NULL
        st1[drop[4:6]] = 1; st1[drop[6]] = 2; st2[drop[7]] = 2   # pMP1 NULL; a bad point on either side
        st1[drop[8]] = 3; st2[drop[9]] = 3                      # GetIndexInKeyFrame < 0
        st1[drop[10]] = 2; st2[drop[10]] = 1; st1[drop[11]] = 1; st2[drop[11]] = 1
        if k == K - 1:
            st2[6:] = 1                                        # at most 6 correspondences: fewer than min_inliers
    return sc


def expected_problems(sc, fix_scale, probability, min_inliers, max_iterations):
    sig = level_sigma2()
    probs = []
    for k in range(sc["K"]):
        keep = np.nonzero((sc["state1"][k] == 0) & (sc["state2"][k] == 0))[0]
        p = dict(x1c=camera_frame(sc["T1"], sc["pos1"][k][keep]), x2c=camera_frame(sc["T2"][k], sc["pos2"][k][keep]),
                 max_err1=(9.210 * sig[sc["oct1"][k][keep]].astype(np.float64)).astype(F),
                 max_err2=(9.210 * sig[sc["oct2"][k][keep]].astype(np.float64)).astype(F), camera1=sc["K1"], camera2=sc["K2"][k],
                 fix_scale=int(fix_scale), min_inliers=min_inliers,
                 iterations=sm.ransac_iterations(len(keep), probability, min_inliers, max_iterations), indices=keep)
        probs.append(p)
    return probs


def run(L, handle, sc, calls, prepare, fix_scale=False, probability=0.99, min_inliers=8, max_iterations=60, seed=12345):
    K, ns, nc = sc["K"], sc["nslots"], len(calls)
    ck = np.array([c[0] for c in calls], np.int32)
    cn = np.array([c[1] for c in calls], np.int32)
    out = dict(ret=np.full(nc, -9, np.int32), no_more=np.full(nc, -9, np.int32), nin=np.full(nc, -9, np.int32), T=np.zeros((nc, 16), F),
               inl=np.full((nc, ns), 9, np.uint8), best_ok=np.full(nc, -9, np.int32), best=np.zeros((nc, 13), F),
               n=np.zeros(K, np.int32), its=np.zeros(K, np.int32), draws=np.zeros((K, max_iterations * 3), np.int32))
    ins = [np.ascontiguousarray(sc[k]) for k in ("state1", "state2", "pos1", "pos2", "oct1", "oct2", "T1", "T2", "K1", "K2")]
    P = lambda a: a.ctypes.data_as(C.c_void_p)                 # noqa: E731
    rc = L.cs_run(handle, K, ns, *[P(a) for a in ins], int(fix_scale), probability, min_inliers, max_iterations, seed, int(prepare), nc,
                  P(ck), P(cn), *[P(out[k]) for k in ("ret", "no_more", "nin", "T", "inl", "best_ok", "best", "n", "its", "draws")])
    assert rc == 0, L.cs_error().decode()
    return out


def check(L, handle, sc, calls, prepare, **kw):
    fix_scale = kw.get("fix_scale", False)
    probability, min_inliers, max_iterations = kw.get("probability", 0.99), kw.get("min_inliers", 8), kw.get("max_iterations", 60)
    got = run(L, handle, sc, calls, prepare, **kw)
    probs = expected_problems(sc, fix_scale, probability, min_inliers, max_iterations)
    assert [len(p["indices"]) for p in probs] == got["n"].tolist()
    assert [p["iterations"] for p in probs] == got["its"].tolist()
    # the draws: at Prepare in list order, otherwise with each solver's first iterate, in call order
    rng = Lcg(kw.get("seed", 12345))
    order = list(range(sc["K"])) if prepare else list(dict.fromkeys(c[0] for c in calls))
    for k in order:
        p = probs[k]
        n = len(p["indices"])
        p["sets"] = rng.draw(n, p["iterations"]) if n >= 3 and n >= min_inliers else np.zeros((p["iterations"], 3), np.int32)
    for k in order:
        p = probs[k]
        if len(p["indices"]) >= min_inliers:
            assert np.array_equal(got["draws"][k][:3 * p["iterations"]], p["sets"].ravel()), k
    solvers = {k: sm.Solver(probs[k], ss.model(probs[k])) for k in order}
    returned = 0
    for c, (k, nit) in enumerate(calls):
        T, no_more, inl, nin = solvers[k].iterate(nit)
        assert got["ret"][c] == (T is not None) and got["no_more"][c] == no_more and got["nin"][c] == nin, (c, k)
        slots = np.zeros(sc["nslots"], np.uint8)
        slots[probs[k]["indices"][inl]] = 1                    # vbInliers[mvnIndices1[i]]
        assert np.array_equal(got["inl"][c], slots), (c, k)
        if T is not None:
            returned += 1
            assert np.array_equal(ss.bits(got["T"][c]), ss.bits(T.ravel())), (c, k)
            assert nin == slots.sum() > min_inliers
        b = solvers[k].best()
        assert got["best_ok"][c] == (b is not None)
        if b is not None:
            want = np.concatenate([b[0].ravel(), b[1], [b[2]]]).astype(F)
            assert np.array_equal(ss.bits(got["best"][c]), ss.bits(want)), (c, k)
    return got, returned


def round_robin(K, rounds):
    return [(k, 5) for _ in range(rounds) for k in range(K)]


def both_ways(L, handle):
    sc = scenario(1)
    got, returned = check(L, handle, sc, round_robin(4, 61), prepare=True)
    assert returned >= 4 and got["no_more"][3] == 1 and got["n"][3] <= 6          # the short candidate is "no more" at its first call
    assert (got["no_more"][-4:] == 1).all()                                       # every solver is exhausted in the end
    # the same solvers, each running alone from its first iterate: solver 2 is called first, so it draws first
    got2, returned2 = check(L, handle, sc, [(2, 5), (0, 5)] + round_robin(4, 61), prepare=False)
    assert returned2 >= 4
    assert not np.array_equal(got["draws"], got2["draws"])                        # other draws: another order of RandomInt calls
    check(L, handle, scenario(2, K=3), [(0, 60), (1, 1), (1, 1), (2, 3), (0, 60), (1, 60)], prepare=True, fix_scale=True, min_inliers=6)


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
