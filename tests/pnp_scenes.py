"""Deterministic scenes for the PnPsolver tests, and the comparisons of a PnPRansac batch with tests/pnp_model.py.  A planted
scene holds a known Tcw, points 2 to 20 m in front of a 640 x 480 TUM camera, image points that are the exact float projections,
planted outliers displaced by 50 px or more, octaves spread over 0 .. 7.  The model's answers are computed once per process:
every problem carries a cache (index tuple -> evaluated hypothesis) that its variants on the same points share."""
from __future__ import annotations

import numpy as np

import pnp_model as pm

D = np.float64
F = np.float32
CAMERA = tuple(float(F(v)) for v in (517.306408, 516.469215, 318.643040, 255.313989))   # TUM1, Frame's floats widened
LEVEL_SIGMA2 = np.array([F(1.2) ** (2 * i) for i in range(8)], F)
RELOC = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5)   # Relocalization's arguments
GPU_N = (4, 5, 63, 64, 65, 129)
GPU_ITERATIONS = (1, 5, 35, 64, 65, 300)
CHUNK = 512            # correspondences k_pnp_inliers stages in LDS at a time
HYP_LANES = 32         # hypotheses per workgroup of k_pnp_hypotheses (half a wave)


def rotation(rng, max_angle):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def project(Tcw, p3dw):
    Xc = p3dw.astype(D) @ Tcw[:3, :3].T + Tcw[:3, 3]
    fu, fv, uc, vc = CAMERA
    return np.stack([uc + fu * Xc[:, 0] / Xc[:, 2], vc + fv * Xc[:, 1] / Xc[:, 2]], 1)


def make(seed, n, outlier_frac=0.3, iterations=None, min_inliers=None, plane=False, identity=False, noise=0.0):
    """noise: standard deviation in px added to the image points of the planted inliers (0 in the planted scenes)"""
    rng = np.random.default_rng(seed)
    Tcw = np.eye(4)
    if not identity:
        Tcw[:3, :3] = rotation(rng, 0.6)
        Tcw[:3, 3] = rng.uniform(-2, 2, 3)
    u = rng.uniform(20, 620, n)
    v = rng.uniform(20, 460, n)
    fu, fv, uc, vc = CAMERA
    x, y = (u - uc) / fu, (v - vc) / fv
    z = 6.0 / (1.0 - 0.5 * x - 0.3 * y) if plane else rng.uniform(2, 20, n)      # the plane z = 6 + 0.5 X + 0.3 Y, tilted
    Xc = np.stack([x * z, y * z, z], 1)
    p3dw = ((Xc - Tcw[:3, 3]) @ Tcw[:3, :3]).astype(F)
    p2d = project(Tcw, p3dw)
    if noise:
        p2d += rng.normal(0.0, noise, p2d.shape)
    nout = int(round(outlier_frac * n))
    planted_inlier = np.ones(n, bool)
    if nout:
        bad = rng.permutation(n)[:nout]
        ang = rng.uniform(0, 2 * np.pi, nout)
        p2d[bad] += (rng.uniform(50, 150, nout) * np.stack([np.cos(ang), np.sin(ang)])).T
        planted_inlier[bad] = False
    octave = (np.arange(n) + seed) % 8
    mi, it = pm.set_ransac_parameters(n, **RELOC) if n > 0 else (RELOC["min_inliers"], 1)
    p = dict(p3dw=p3dw, p2d=p2d.astype(F), max_err=pm.max_error(LEVEL_SIGMA2[octave]), camera=CAMERA,
             min_inliers=mi if min_inliers is None else min_inliers, iterations=it if iterations is None else iterations,
             truth=Tcw, planted_inlier=planted_inlier, seed=seed, plane=plane, cache={})
    p["sets"] = pm.Lcg(seed).draw(n, p["iterations"]) if n >= 4 else None
    return p


def variant(p, **kw):
    q = dict(p)
    q.update(kw)
    if any(k in kw for k in ("p3dw", "p2d", "max_err", "camera")):
        q["cache"] = {}
    return q


def launches(p):
    return len(p["p3dw"]) >= p["min_inliers"]


def solver(p, prim=pm.Own):
    return pm.Solver(p, prim, p["cache"] if prim is pm.Own else p.setdefault("cache_lapack", {}))


_SCENES = {}


def _once(name, fn):
    if name not in _SCENES:
        _SCENES[name] = fn()
    return _SCENES[name]


def planted_scenes():
    """general scenes at 0 / 30 / 45 % outliers, the planar scene (25 %), the identity scene (20 %)"""
    return _once("planted", lambda: [make(1, 40, 0.0), make(2, 60, 0.3), make(5, 100, 0.45), make(4, 48, 0.25, plane=True),
                                     make(6, 30, 0.2, identity=True)])


def two_pose_scene():
    """12 points seen from pose A followed by 30 points seen from pose B, min_inliers = 12.  sets[0] is drawn among A's points
    and counts exactly 12, so it qualifies, becomes the best, and its Refine (12 again, not MORE than 12) fails; sets[1] is
    drawn among B's points and counts 30, so the best moves and Refine succeeds.  The two sets are the first of an Lcg's draws
    that the model counts that way; the rest of the list are ordinary draws."""
    def build():
        a, b = make(300, 12, 0.0), make(301, 30, 0.0)
        p = dict(p3dw=np.concatenate([a["p3dw"], b["p3dw"]]), p2d=np.concatenate([a["p2d"], b["p2d"]]),
                 max_err=np.concatenate([a["max_err"], b["max_err"]]), camera=CAMERA, min_inliers=12, iterations=6,
                 truth=b["truth"], planted_inlier=np.arange(42) >= 12, seed=300, plane=False, cache={})
        sv = pm.Solver(p, pm.Own, p["cache"])
        first = next(s for s in pm.Lcg(300).draw(12, 30) if sv._eval(s).count == 12)
        second = next(s + 12 for s in pm.Lcg(301).draw(30, 30) if sv._eval(s + 12).count == 30)
        p["sets"] = np.concatenate([[first, second], pm.Lcg(302).draw(42, 4)]).astype(np.int32)
        return p
    return _once("two_pose", build)


def size_problems():
    """N over the mask-word boundaries x iteration counts over the wave / workgroup boundaries of both kernels"""
    def build():
        out = []
        for j, n in enumerate(GPU_N):
            it = GPU_ITERATIONS[j]
            out.append(make(100 + j, n, 0.0 if n < 8 else 0.25, iterations=it, min_inliers=4 if n < 20 else None))
        # the partition of k_pnp_hypotheses: HYP_LANES hypotheses per workgroup (half a wave): 31, 32, 33 iterations
        out += [make(110, 20, 0.2, iterations=HYP_LANES - 1), make(111, 20, 0.2, iterations=HYP_LANES),
                make(112, 20, 0.2, iterations=HYP_LANES + 1)]
        return out
    return _once("sizes", build)


def chunk_problems():
    return _once("chunks", lambda: [make(120 + j, n, 0.3, iterations=5) for j, n in enumerate((CHUNK - 1, CHUNK, CHUNK + 1))])


def mixed_call():
    """different N and iteration counts, and two problems that launch nothing (the second without sets)"""
    def build():
        small = make(131, 6, 0.0, iterations=7, min_inliers=10)
        return [make(130, 30, 0.2, iterations=9), small, make(132, 70, 0.3, iterations=33),
                variant(make(133, 3, 0.0, iterations=4, min_inliers=10), sets=None), make(134, 21, 0.1, iterations=2)]
    return _once("mixed", build)


def poisoned():
    """outside the contract: inf, nan, 1e30 and 0.0 in a drawn point and in an undrawn point"""
    def build():
        base = make(140, 24, 0.2, iterations=6, min_inliers=8)
        drawn = int(base["sets"][0, 0])
        undrawn = int(np.setdiff1d(np.arange(24), base["sets"].reshape(-1))[0]) if len(
            np.setdiff1d(np.arange(24), base["sets"].reshape(-1))) else None
        out = []
        for poison in (np.inf, np.nan, 1e30, 0.0):
            for idx in (drawn, undrawn):
                if idx is None:
                    continue
                x = base["p3dw"].copy()
                x[idx] = poison
                out.append(variant(base, p3dw=x))
        return out
    return _once("poisoned", build)


# ------------------------------------------------------------------------------------------------ comparisons
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_batch_equals_model(rb, problems, what):
    """every stored iteration: the double R | t, the float Tcw, N, the mask and the count"""
    for k, p in enumerate(problems):
        counts = rb.counts(k)
        if not launches(p):
            assert len(counts) == 0, (what, k)
            continue
        sv = solver(p)
        assert len(counts) == len(sv.sets), (what, k)
        for i in range(len(sv.sets)):
            h = sv.hyp(i)
            rt, T, N, mask = rb.hypothesis(k, i)
            where = (what, k, i)
            assert (bits(rt) == bits(np.concatenate([h.R.reshape(-1), h.t]))).all(), where
            assert (bits(T) == bits(h.Tcw.reshape(-1))).all(), where
            assert N == h.N, where
            assert (mask == h.mask).all() and counts[i] == h.count, where


def assert_replay_equals_model(rb, problems, schedule, what, extra_seed=9000):
    """every iterate return against the model's Solver, and mBestTcw / mnBestInliers after every call.  Default schedule: the
    round-robin of Relocalization with iterate(5) until every solver has said no_more.  A -2 is met with further draws (Lcg of
    extra_seed + k) appended to both sides."""
    solvers = [solver(p) for p in problems]
    extra = [pm.Lcg(extra_seed + k) for k in range(len(problems))]
    if schedule is None:
        schedule = []
        live = list(range(len(problems)))
        shadow = [solver(variant(p, cache=p["cache"])) for p in problems]
        guard = 0
        while live and guard < 400:
            guard += 1
            for k in list(live):
                r = shadow[k].iterate(5)
                if r is None:                                   # past its stored sets: the explicit -2 tests cover that
                    live.remove(k)
                    continue
                schedule.append((k, 5))
                if r[1]:
                    live.remove(k)
    for k, nit in schedule:
        while True:
            before = rb.counts(k).copy()
            r, T, no_more, inl, nin = rb.iterate_raw(k, nit)
            m = solvers[k].iterate(nit)
            where = (what, k, nit, solvers[k].done)
            if m is None:
                assert r == -2, where
                assert (rb.counts(k) == before).all(), where
                more = extra[k].draw(len(problems[k]["p3dw"]), max(nit, 1))
                rb.append(k, more)
                solvers[k].append(more)
                continue
            break
        mT, mno, minl, mnin = m
        assert r == (1 if mT is not None else 0), where
        assert no_more == mno and nin == mnin and (inl == minl).all(), where
        if mT is not None:
            assert (bits(T.reshape(-1)) == bits(mT.reshape(-1))).all(), where
        if solvers[k].best is not None:
            bT, bn, bit = rb.best(k)
            assert bn == solvers[k].best_inliers and bit == solvers[k].best_it, where
            assert (bits(bT.reshape(-1)) == bits(solvers[k].best.Tcw.reshape(-1))).all(), where
    return solvers
