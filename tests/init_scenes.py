"""Problems for the Initializer H / F RANSAC tests (tests/test_init_cpu.py, tests/test_init_gpu.py): planted two-view scenes with a
known model and known outliers, the size lists of the kernels' partitions, the degenerate and the nothing-scores problems, and
the comparison of a batch with tests/init_model.py, whose answers are computed once per process and kept."""
import numpy as np

import init_model as im

F = np.float32
K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1]])
HYP_LANES, SCORE_LANES, CHUNK = 64, 64, 256          # ORBX_INIT_HYP_LANES, ORBX_INIT_SCORE_LANES, ORBX_INIT_CHUNK
GPU_N = (8, 9, 63, 64, 65, 129, CHUNK - 1, CHUNK, CHUNK + 1)
GPU_ITERATIONS = (1, 200, HYP_LANES - 1, HYP_LANES, HYP_LANES + 1)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def rot(axis, deg):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def project(R, t, P):
    c = P @ R.T + t
    return (c[:, :2] / c[:, 2:]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]


def draw_sets(rng, n, iterations):
    return np.stack([rng.choice(n, 8, replace=False) for _ in range(iterations)]).astype(np.int32)


def make(seed, n, kind="general", outliers=0.25, iterations=200, extra1=0, extra2=0, sigma=1.0, models=im.H | im.FUND, cluster=False):
    """a two-view scene: kind = "plane", "general" or "rotation"; n matches of which a share are displaced by at least 20 px in
    frame 2 (against the epipolar line too, so they are outliers of F as well as of H); extra1 / extra2 unmatched keypoints, spread
    over the image or (cluster) packed into one corner far from the matched ones; the keypoint order of both frames is shuffled"""
    rng = np.random.RandomState(seed)
    R, t = rot([0.2, 1.0, 0.1], 6.0), np.array([0.5, 0.05, 0.1])
    if kind == "rotation":
        t = np.zeros(3)
    P = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.8, 1.8, n), rng.uniform(4.0, 9.0, n)], axis=1)
    if kind == "plane":
        P[:, 2] = 6.0 + 0.3 * P[:, 0] - 0.2 * P[:, 1]
    x1, x2 = project(np.eye(3), np.zeros(3), P), project(R, t, P)
    nout = int(round(outliers * n))
    bad = np.zeros(n, bool)
    bad[rng.choice(n, nout, replace=False)] = True
    Kinv = np.linalg.inv(K)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ftrue = Kinv.T @ tx @ R @ Kinv
    for i in np.flatnonzero(bad):
        while True:
            d = rng.uniform(-1, 1, 2)
            d = d / np.linalg.norm(d) * rng.uniform(20.0, 60.0)
            if kind == "rotation":
                break
            line = Ftrue @ np.array([x1[i, 0], x1[i, 1], 1.0])
            q = x2[i] + d
            if abs(line[0] * q[0] + line[1] * q[1] + line[2]) / np.hypot(line[0], line[1]) >= 10.0:
                break
        x2[i] = x2[i] + d
    if cluster:
        e1 = rng.uniform([600, 10], [635, 40], (extra1, 2))
        e2 = rng.uniform([5, 440], [40, 475], (extra2, 2))
    else:
        e1, e2 = rng.uniform([0, 0], [640, 480], (extra1, 2)), rng.uniform([0, 0], [640, 480], (extra2, 2))
    o1, o2 = rng.permutation(n + extra1), rng.permutation(n + extra2)
    keys1, keys2 = np.concatenate([x1, e1])[o1].astype(F), np.concatenate([x2, e2])[o2].astype(F)
    matches = np.stack([np.argsort(o1)[:n], np.argsort(o2)[:n]], axis=1).astype(np.int32)
    return dict(keys1=keys1, keys2=keys2, matches=matches, sigma=sigma, iterations=iterations,
                sets=draw_sets(rng, n, iterations) if n >= 8 else None, models=models, planted_inlier=~bad, kind=kind, seed=seed)


def variant(p, **kw):
    q = dict(p)
    q.update(kw)
    q.pop("_model", None)
    return q


def launches(p):
    return len(p["matches"]) >= 8 and p.get("models", 3) != 0


_cache = {}


def cached(name, fn):
    if name not in _cache:
        _cache[name] = fn()
    return _cache[name]


def planted_scenes():
    """plane, general 3-D scene, pure rotation; the last has unmatched keypoints clustered in a corner of each frame"""
    return cached("planted", lambda: [make(1, 120, "plane", extra1=40, extra2=25), make(2, 150, "general", extra1=10, extra2=60),
                                      make(3, 100, "rotation", extra1=30, extra2=30),
                                      make(4, 90, "general", extra1=300, extra2=200, cluster=True)])


def degenerate():
    """iteration 0 draws eight matches whose keypoints coincide, iteration 1 eight collinear ones, iteration 2 a NaN keypoint is
    NOT drawn anywhere: the rest of the problem is the general scene"""
    def build():
        p = make(5, 80, "general", iterations=12, extra1=5, extra2=5)
        k1, k2, m, sets = p["keys1"].copy(), p["keys2"].copy(), p["matches"], p["sets"].copy()
        for i in range(8):                                       # matches 0 .. 7: one and the same point in both frames
            k1[m[i, 0]], k2[m[i, 1]] = k1[m[0, 0]], k2[m[0, 1]]
        for i in range(8, 16):                                   # matches 8 .. 15: on one line in both frames
            s = F(i - 8)
            k1[m[i, 0]] = (F(100) + F(20) * s, F(80) + F(10) * s)
            k2[m[i, 1]] = (F(140) + F(20) * s, F(90) + F(10) * s)
        sets[0], sets[1] = np.arange(8), np.arange(8, 16)
        for i in range(2, len(sets)):                             # the other draws avoid the sixteen planted matches
            sets[i] = 16 + (sets[i] % 64)
            while len(set(sets[i])) < 8:
                sets[i] = 16 + np.random.RandomState(i).choice(64, 8, replace=False)
        return variant(p, keys1=k1, keys2=k2, sets=sets)
    return cached("degenerate", build)


def none_scenes():
    """nothing scores: (a) a sigma so small that only an exactly zero distance could; (b) every keypoint of frame 2 is NaN, so
    every chi-square is NaN, every mask is all-true (bIn is left alone) and every score is NaN; (c) fewer than 8 matches"""
    def build():
        a = variant(make(6, 40, "general", iterations=20, outliers=1.0), sigma=1e-12)
        b = make(7, 30, "general", iterations=9)
        b = variant(b, keys2=np.full_like(b["keys2"], np.nan))
        c = make(8, 7, "general", iterations=5)
        return [a, b, c]
    return cached("none", build)


def size_problems():
    """n around the mask words and the LDS chunk of k_init_scores, iterations around the workgroup of k_init_hypotheses (and of
    k_init_scores, which takes 64 hypotheses each), H only, F only and both, n1 != n2 and both larger than n"""
    def build():
        out = []
        for i, n in enumerate(GPU_N):
            out.append(make(20 + i, n, "general", iterations=(5, 3, 7)[i % 3], extra1=3 + i, extra2=12 - i, models=(3, 1, 2)[i % 3]))
        for i, it in enumerate(GPU_ITERATIONS):
            out.append(make(40 + i, 24, "plane", iterations=it, extra1=2, extra2=9, models=(3, 1, 2, 3, 3)[i]))
        out.append(make(50, 40, "general", iterations=200, extra1=5, extra2=1, models=1))
        out.append(make(51, 40, "general", iterations=65, extra1=0, extra2=4, models=2))
        return out
    return cached("sizes", build)


def mixed_call():
    """14 problems of different n, iteration counts and models in one call, two of which launch nothing"""
    def build():
        spec = [(70, 5, 3), (5, 4, 3), (9, 64, 1), (0, 3, 3), (130, 33, 2), (64, 1, 3), (8, 2, 2), (257, 6, 3), (33, 31, 1), (100, 65, 3),
                (63, 10, 2), (12, 127, 3), (256, 2, 1), (65, 9, 3)]
        return [make(60 + i, n, ("general", "plane", "rotation")[i % 3], iterations=it, extra1=i, extra2=14 - i, models=mo)
                for i, (n, it, mo) in enumerate(spec)]
    return cached("mixed", build)


def model_of(p):
    if "_model" not in p:
        p["_model"] = im.solve(p)
    return p["_model"]


def assert_batch_equals_model(rb, problems, what=""):
    """everything the library reports for every problem of the batch against tests/init_model.py, bit for bit"""
    assert len(rb) == len(problems)
    for k, p in enumerate(problems):
        tag = f"{what}: problem {k}"
        mo = model_of(p)
        T1, T2 = rb.normalization(k)
        assert np.array_equal(bits(T1), bits(mo["T1"])) and np.array_equal(bits(T2), bits(mo["T2"])), tag
        r = rb.result(k)
        n = len(p["matches"])
        for model, name in ((im.H, "H"), (im.FUND, "F")):
            sc = rb.scores(k, model)
            per = mo["per"].get(model)
            if per is None:
                assert len(sc) == 0 and r["it" + name] == -1 and not r["inliers" + name].any() and bits(r["S" + name]) == 0, tag
                continue
            assert len(sc) == p["iterations"], tag
            assert np.array_equal(bits(sc), bits(per["scores"])), (tag, name, "scores")
            for it in range(p["iterations"]):
                M, Mi, s, mask = rb.hypothesis(k, model, it)
                assert np.array_equal(bits(M), bits(per["M"][it])), (tag, name, it, "matrix")
                assert np.array_equal(bits(Mi), bits(per["Minv"][it])), (tag, name, it, "inverse")
                assert bits(s) == bits(per["scores"][it]) and np.array_equal(mask, per["masks"][it]), (tag, name, it, "mask")
            best = mo["it" + name]
            assert r["it" + name] == best and bits(r["S" + name]) == bits(mo["S" + name]), (tag, name, "best")
            want_M = per["M"][best] if best >= 0 else np.zeros((3, 3), F)
            want_mask = per["masks"][best] if best >= 0 else np.zeros(n, bool)
            assert np.array_equal(bits(r[name + "21"]), bits(want_M)) and np.array_equal(r["inliers" + name], want_mask), (tag, name)
        assert bits(r["RH"]) == bits(mo["RH"]) and r["model"] == mo["model"], (tag, "RH, model")
