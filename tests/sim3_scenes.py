"""Scenes for the Sim3Solver tests: two keyframes that see the same points, related by a known Sim3 (scale 0.7 ... 1.4),
sub-pixel noise, gross outliers; the reference's draws (three indices without replacement from a shrinking list,
src/Sim3Solver.cc:237-258) from a seeded generator; the size lists of the CPU and GPU tests; the model's answers, computed once
per process; and the comparison of a library batch with them, bit for bit."""
import functools

import numpy as np

import sim3_model as sm

F = np.float32
CAMERA1 = np.array([517.3, 516.5, 318.6, 255.3], F)
CAMERA2 = np.array([535.4, 539.2, 320.1, 247.6], F)
SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)], np.float64).astype(F)       # mvLevelSigma2


def max_err(levels):
    """mvnMaxError: 9.210 * sigmaSquare, the product in double, stored as float (:114-115)"""
    return (9.210 * SIGMA2[levels].astype(np.float64)).astype(F)


def draws(rng, n, iterations):
    """the index triples iterate() would draw: vAvailableIndices = all, three times RandomInt(0, size - 1), swap with the back"""
    out = np.zeros((iterations, 3), np.int32)
    for i in range(iterations):
        avail = list(range(n))
        for c in range(3):
            r = int(rng.integers(0, len(avail)))
            out[i, c] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def make(seed, n, iterations=None, outlier_frac=0.3, noise_px=0.3, fix_scale=False, min_inliers=None, scale=None):
    """x1c = s R x2c + t + noise for the planted inliers, anything for the planted outliers"""
    rng = np.random.default_rng(1000 + seed)
    s = 1.0 if fix_scale else (float(rng.uniform(0.7, 1.4)) if scale is None else scale)
    R = rotation(rng.normal(size=3), rng.uniform(0.05, 0.5))
    t = rng.uniform(-0.4, 0.4, 3)
    x2 = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3.0, 7.0, n)], axis=1)
    x1 = s * x2 @ R.T + t
    x1 = x1 + rng.normal(size=(n, 3)) * (noise_px * x1[:, 2:3] / 520.0)          # about noise_px pixels in image 1
    planted_out = np.zeros(n, bool)
    nout = int(round(outlier_frac * n))
    if nout:
        planted_out[rng.choice(n, nout, replace=False)] = True
        x1[planted_out] = np.stack([rng.uniform(-1.5, 1.5, nout), rng.uniform(-1.0, 1.0, nout), rng.uniform(2.0, 8.0, nout)], axis=1)
    l1, l2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    if min_inliers is None:
        min_inliers = min(20, max(3, n // 3))
    if iterations is None:
        iterations = sm.ransac_iterations(n, 0.99, min_inliers, 300)
    p = dict(x1c=x1.astype(F), x2c=x2.astype(F), max_err1=max_err(l1), max_err2=max_err(l2), camera1=CAMERA1, camera2=CAMERA2,
             fix_scale=int(fix_scale), min_inliers=int(min_inliers), iterations=int(iterations))
    p["sets"] = draws(rng, n, iterations) if n >= 3 else np.zeros((iterations, 3), np.int32)
    p["planted_inlier"] = ~planted_out
    p["truth"] = (s, R, t)
    return p


def variant(p, **kw):
    q = dict(p)
    q.update(kw)
    return q


_CACHE = {}


def model(p):
    """sm.evaluate(p), once per process for a given problem"""
    key = (p["x1c"].tobytes(), p["x2c"].tobytes(), p["max_err1"].tobytes(), p["max_err2"].tobytes(), np.asarray(p["sets"]).tobytes(),
           np.asarray(p["camera1"]).tobytes(), np.asarray(p["camera2"]).tobytes(), p["fix_scale"], p["min_inliers"], p["iterations"])
    if key not in _CACHE:
        _CACHE[key] = sm.evaluate(p)
    return _CACHE[key]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_batch_equals_model(rb, problems, what=""):
    """hypothesis floats as uint32, masks and counts of every stored iteration of a library batch"""
    assert len(rb) == len(problems)
    for k, p in enumerate(problems):
        want = model(p)
        counts = rb.counts(k)
        if want is None:
            assert len(counts) == 0, (what, k)
            continue
        hyps, masks, cnt = want
        assert np.array_equal(counts, cnt), (what, k, np.nonzero(counts != cnt)[0][:5])
        for i in range(p["iterations"]):
            h, m = rb.hypothesis(k, i)
            assert np.array_equal(bits(h), bits(hyps[i])), (what, k, i, h, hyps[i])
            assert np.array_equal(m, masks[i]), (what, k, i)


def assert_replay_equals_model(rb, problems, schedule=None, what=""):
    """every iterate return and the best state after every call; schedule = (k, n_iterations) pairs, or None: iterate(5) round
    robin until every solver has reported no_more"""
    solvers = [sm.Solver(p, model(p)) for p in problems]

    def call(k, nit):
        T, no_more, inl, nin = rb.iterate(k, nit)
        wT, wno, winl, wnin = solvers[k].iterate(nit)
        assert (T is None) == (wT is None) and no_more == wno and nin == wnin, (what, k, nit)
        assert np.array_equal(inl, winl), (what, k)
        if T is not None:
            assert np.array_equal(bits(T), bits(wT)), (what, k)
        wb = solvers[k].best()
        if wb is not None:
            R, t, s = rb.best(k)
            assert np.array_equal(bits(R), bits(wb[0])) and np.array_equal(bits(t), bits(wb[1])) and bits(s) == bits(wb[2]), (what, k)
        return no_more

    if schedule is not None:
        for k, nit in schedule:
            call(k, nit)
        return solvers
    live = set(range(len(problems)))
    while live:
        for k in sorted(live):
            if call(k, 5):
                live.discard(k)
    return solvers


# the sizes at which the kernels can go wrong: mask word boundaries and the tail; wave and workgroup boundaries of the iterations
GPU_N = (3, 20, 63, 64, 65, 129)
GPU_ITERATIONS = (1, 5, 64, 65, 300)


@functools.lru_cache(maxsize=None)
def planted_scenes():
    """seeds chosen so that the model alone satisfies the planted-scene properties (tests/test_sim3_cpu.py asserts them)"""
    return (make(1, 100), make(2, 60, outlier_frac=0.4), make(3, 40, fix_scale=True), make(4, 150, outlier_frac=0.2, iterations=40))


@functools.lru_cache(maxsize=None)
def size_problems():
    """N x iterations of the GPU size lists, as problems of <= 16 per call, each call mixing sizes"""
    probs = []
    for a, n in enumerate(GPU_N):
        for b, it in enumerate(GPU_ITERATIONS):
            if it == 300 and n not in (20, 129):               # 300 iterations twice is enough for the workgroup table
                continue
            probs.append(make(100 + 10 * a + b, n, iterations=it, min_inliers=3 if n < 20 else 6, fix_scale=(a + b) % 3 == 0))
    return tuple(probs)


@functools.lru_cache(maxsize=None)
def chunk_problems():
    """N at and past the 512 correspondences k_sim3_inliers stages in LDS at a time"""
    return (make(300, 512, iterations=5, min_inliers=20), make(301, 513, iterations=6, min_inliers=20),
            make(302, 1100, iterations=3, min_inliers=20, fix_scale=True))


def degenerate():
    """collinear triples, one point three times, a point behind camera 2, a point at z == 0 of its own camera"""
    p = make(41, 40, iterations=6, min_inliers=6)
    x1, x2 = p["x1c"].copy(), p["x2c"].copy()
    x2[1] = x2[0] + F(0.5) * (x2[2] - x2[0])                   # 0, 1, 2 collinear in frame 2 ...
    x1[1] = x1[0] + F(0.5) * (x1[2] - x1[0])                   # ... and in frame 1
    x2[9] = (0.2, -0.1, -3.0)                                  # behind camera 2, finite terms
    x1[10] = (0.1, 0.3, 0.0)                                   # z == 0 in its own camera: mvP1im1 is not finite
    sets = p["sets"].copy()
    sets[0] = (0, 1, 2)
    sets[1] = (4, 4, 4)                                        # one point three times: Pr = 0, N = 0, the quaternion is (1, 0, 0, 0)
    sets[2] = (4, 4, 7)
    sets[3] = (5, 6, 5)
    sets[4] = [i for i in np.nonzero(p["planted_inlier"])[0] if i not in (0, 1, 2, 9, 10)][:3]   # and one sound triple
    return variant(p, x1c=x1, x2c=x2, sets=sets)


def mixed_call():
    """different N and iteration counts in one call, one problem that launches nothing, one with n = 0"""
    return [make(200, 65, iterations=5, min_inliers=6), make(201, 10, iterations=7, min_inliers=20),
            make(202, 129, iterations=65, min_inliers=6), make(203, 0, iterations=3, min_inliers=20),
            make(204, 3, iterations=1, min_inliers=3), make(205, 64, iterations=64, min_inliers=6)]
