"""Problems for the ReconstructH / ReconstructF tests (tests/test_recon_cpu.py, tests/test_recon_gpu.py, tests/test_compat_recon.py):
two-view scenes with a planted motion whose H21 or F21 is formed from that motion in float64 and whose mask is the planted one,
chosen so that tests/recon_model.py ALONE shows each case (test_recon_cpu.py asserts that on the model's answers), and the
comparison of a batch with the model, whose answers are computed once per process and kept."""
import numpy as np

import init_scenes as isc
import recon_model as rm

F = np.float32
K = isc.K
K4 = (500.0, 500.0, 320.0, 240.0)
bits = isc.bits
GPU_N = (1, 8, 63, 64, 65, 129)                      # the ballot words of k_init_check_rt and the tail
WINNER_COUNTS = (0, 1, 50, 51, 52, 80)               # nGood of the winner on both sides of idx = min(50, size - 1)


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def scene(seed, n, kind, R=None, t=None, outliers=0.0, model=None, extra1=4, extra2=7, **kw):
    """n matches of a planted motion (R, t): kind "plane" (z = 6 + 0.3 x - 0.2 y) or "general"; a share of the matches is
    displaced by 20 to 60 px in frame 2 and left out of the mask; the keypoint order of both frames is shuffled"""
    rng = np.random.RandomState(seed)
    R = isc.rot([0.2, 1.0, 0.1], 6.0) if R is None else R
    t = np.array([0.5, 0.05, 0.1]) if t is None else np.asarray(t, float)
    P = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.8, 1.8, n), rng.uniform(4.0, 9.0, n)], axis=1)
    nrm, d = np.array([-0.3, 0.2, 1.0]), 6.0                     # the plane nrm . X = d
    if kind == "plane":
        P[:, 2] = 6.0 + 0.3 * P[:, 0] - 0.2 * P[:, 1]
    x1, x2 = isc.project(np.eye(3), np.zeros(3), P), isc.project(R, t, P)
    bad = np.zeros(n, bool)
    bad[rng.choice(n, int(round(outliers * n)), replace=False)] = True
    for i in np.flatnonzero(bad):
        v = rng.uniform(-1, 1, 2)
        x2[i] = x2[i] + v / np.linalg.norm(v) * rng.uniform(20.0, 60.0)
    Kinv = np.linalg.inv(K)
    model = model or (rm.H if kind == "plane" else rm.FUND)
    M = K @ (R + np.outer(t, nrm) / d) @ Kinv if model == rm.H else Kinv.T @ skew(t) @ R @ Kinv
    M = M / np.abs(M).max()
    e1, e2 = rng.uniform([0, 0], [640, 480], (extra1, 2)), rng.uniform([0, 0], [640, 480], (extra2, 2))
    o1, o2 = rng.permutation(n + extra1), rng.permutation(n + extra2)
    keys1, keys2 = np.concatenate([x1, e1])[o1].astype(F), np.concatenate([x2, e2])[o2].astype(F)
    matches = np.stack([np.argsort(o1)[:n], np.argsort(o2)[:n]], axis=1).astype(np.int32)
    p = dict(keys1=keys1, keys2=keys2, matches=matches, inliers=~bad, model=model, M=M.astype(F), K=K4, sigma=1.0,
             min_parallax=1.0, min_triangulated=50, R_true=R, t_true=t, kind=kind, seed=seed)
    p.update(kw)
    return p


def variant(p, **kw):
    q = dict(p)
    q.update(kw)
    q.pop("_model", None)
    return q


def only(p, count, seed=0):
    """the same problem with exactly `count` of its planted inliers left in the mask"""
    idx = np.flatnonzero(p["inliers"])
    keep = np.random.RandomState(seed).choice(idx, count, replace=False)
    m = np.zeros(len(p["inliers"]), bool)
    m[keep] = True
    return variant(p, inliers=m)


def cases():
    """name -> problem; what each must show is asserted on the model in tests/test_recon_cpu.py"""
    def build():
        c = {}
        c["plane_h"] = scene(101, 120, "plane", R=isc.rot([0.2, 1.0, 0.1], -20.0), t=[2.0, 0.0, 0.5], outliers=0.25)
        c["general_f"] = scene(102, 150, "general", outliers=0.25)
        c["rotation_h"] = scene(103, 100, "plane", t=[0.0, 0.0, 0.0], outliers=0.2)
        c["low_parallax_f"] = scene(104, 150, "general", R=isc.rot([0.1, 1.0, 0.0], 1.0), t=[0.07, 0.0, 0.0], outliers=0.2)
        c["tie_f"] = scene(105, 90, "general", R=isc.rot([0.1, 1.0, 0.0], 1.0), t=[0.0005, 0.0, 0.0])
        g = scene(106, 140, "general")
        for k in WINNER_COUNTS[1:]:
            c[f"winner_{k}"] = only(g, k, seed=k)
        o = scene(107, 60, "general", outliers=0.5)
        c["winner_0"] = variant(o, inliers=~o["inliers"], sigma=0.01)   # only the displaced matches are left in the mask
        c["behind_f"] = behind()
        c["nonfinite_repeated_f"] = nonfinite_repeated()
        c["all_false"] = variant(scene(108, 40, "general"), inliers=np.zeros(40, bool))
        c["n0"] = variant(scene(109, 10, "general"), matches=np.zeros((0, 2), np.int32), inliers=np.zeros(0, bool))
        c["plane_as_f"] = scene(110, 70, "plane", model=rm.FUND)
        c["general_as_h"] = scene(111, 70, "general", model=rm.H)
        return c
    return isc.cached("recon_cases", build)


def behind():
    """match 0 is a point 5000 units BEHIND both cameras: the DLT recovers it with z < 0, its rays are parallel to a few parts in
    a million (cosParallax >= 0.99998), so neither depth test rejects it and it is counted without being flagged"""
    p = scene(112, 80, "general")
    k1, k2, m = p["keys1"].copy(), p["keys2"].copy(), p["matches"]
    P = np.array([[300.0, -200.0, -5000.0]])
    k1[m[0, 0]] = isc.project(np.eye(3), np.zeros(3), P)[0]
    k2[m[0, 1]] = isc.project(p["R_true"], p["t_true"], P)[0]
    return variant(p, keys1=k1, keys2=k2)


def nonfinite_repeated():
    """matches 3 and 40 share their `first` keypoint, and so do 5 and 41.  Match 40 pairs it with a NaN keypoint of frame 2:
    its point is not finite and vbTriangulated[first], set by match 3, is reset.  Match 41 repeats match 5's pair exactly."""
    p = scene(113, 60, "general", extra2=9)
    k2, m = p["keys2"].copy(), p["matches"].copy()
    spare = np.setdiff1d(np.arange(len(k2)), m[:, 1])[0]
    k2[spare] = np.nan
    m[40] = (m[3, 0], spare)
    m[41] = m[5]
    return variant(p, keys2=k2, matches=m)


def size_problems():
    """n around the ballot words, every match an inlier; both models"""
    def build():
        out = []
        for i, n in enumerate(GPU_N):
            out.append(scene(130 + i, n, "general", min_triangulated=0))
            out.append(scene(140 + i, n, "plane", min_triangulated=0))
        return out
    return isc.cached("recon_sizes", build)


def mixed_call():
    """both models with different n in one call, two problems that launch nothing"""
    def build():
        c = cases()
        return [c["plane_h"], c["all_false"], c["general_f"], scene(150, 33, "plane", outliers=0.1), c["n0"],
                scene(151, 200, "general", outliers=0.3), c["rotation_h"], c["winner_51"], scene(152, 70, "plane", model=rm.FUND)]
    return isc.cached("recon_mixed", build)


def ransac_problems():
    """problems of the H / F RANSAC for the fused call: the planted scenes of tests/init_scenes.py, a problem that scores nothing
    (ORBX_INIT_NONE), one with n < 8, H only and F only"""
    def build():
        pl = list(isc.planted_scenes())
        return [pl[0], pl[1], isc.none_scenes()[0], pl[2], isc.none_scenes()[2], isc.variant(pl[3], models=rm.FUND),
                isc.variant(pl[0], models=rm.H), isc.make(9, 40, "general", iterations=30, extra1=3, extra2=2)]
    return isc.cached("recon_ransac", build)


def camera():
    return dict(K=K4, min_parallax=1.0, min_triangulated=50)


def from_ransac(p, r, cam):
    """the stand-alone problem that continues a RANSAC result r (InitializerRansac.result) of problem p"""
    model = r["model"] if r["model"] != rm.im.NONE else rm.FUND
    none = r["model"] == rm.im.NONE
    M = np.zeros((3, 3), F) if none else (r["H21"] if model == rm.H else r["F21"])
    inl = np.zeros(len(p["matches"]), bool) if none else (r["inliersH"] if model == rm.H else r["inliersF"])
    return dict(keys1=p["keys1"], keys2=p["keys2"], matches=p["matches"], inliers=inl, model=model, M=M, K=cam["K"],
                sigma=p["sigma"], min_parallax=cam["min_parallax"], min_triangulated=cam["min_triangulated"])


def model_of(p):
    if "_model" not in p:
        p["_model"] = rm.solve(p)
    return p["_model"]


def assert_result_equals(r, hyps, mo, tag):
    assert r["ok"] == mo["ok"] and r["chosen"] == mo["chosen"] and r["N"] == mo["N"], (tag, r["ok"], mo["ok"], r["chosen"], mo["chosen"])
    assert np.array_equal(bits(r["R21"]), bits(mo["R21"])) and np.array_equal(bits(r["t21"]), bits(mo["t21"])), (tag, "R21, t21")
    assert np.array_equal(r["status"], mo["status"]), (tag, "status", np.flatnonzero(r["status"] != mo["status"])[:8])
    assert np.array_equal(bits(r["points"]), bits(mo["points"])), (tag, "points")
    assert len(hyps) == len(mo["hyp"]), tag
    for i, (h, w) in enumerate(zip(hyps, mo["hyp"])):
        assert h["valid"] == w["valid"] and h["nGood"] == w["nGood"], (tag, i, h["nGood"], w["nGood"])
        for f in ("R", "t", "n", "cosine", "parallax"):
            assert np.array_equal(bits(h[f]), bits(w[f])), (tag, i, f, h[f], w[f])


def assert_batch_equals_model(rc, problems, what=""):
    """everything the library reports for every problem of the batch against tests/recon_model.py, bit for bit"""
    assert len(rc) == len(problems)
    for k, p in enumerate(problems):
        mo = model_of(p)
        hyps = [rc.hypothesis(k, i) for i in range(len(mo["hyp"]))]
        assert_result_equals(rc.result(k), hyps, mo, f"{what}: problem {k}")
