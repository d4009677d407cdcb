"""Seeded scenes for Optimizer::OptimizeEssentialGraph (orbx_optimize_essential_graph_batch): a set of Sim3 keyframe poses that
agree with each other (the "odometry", passed as NonCorrectedSim3 so that every step-4 edge measures it), start estimates Scw
= a small Sim3 perturbation of them, a graph, and map points with their reference vertices.  Each scene is the dict
optimizer.optimize_essential_graph_batch takes."""
import numpy as np


def sim3_row(axis_angle, t, s):
    a = np.asarray(axis_angle, np.float64)
    th = np.linalg.norm(a)
    q = np.array([0.0, 0.0, 0.0, 1.0]) if th == 0 else np.concatenate([np.sin(th / 2) * a / th, [np.cos(th / 2)]])
    return np.concatenate([q, np.asarray(t, np.float64), [float(s)]])


def compose(a, b):
    """a * b of two rows (plain float64 algebra: the scenes only need poses that are roughly consistent)"""
    def rot(q, v):
        u = 2 * np.cross(q[:3], v)
        return v + q[3] * u + np.cross(q[:3], u)
    qa, qb = a[:4], b[:4]
    w = qa[3] * qb[3] - qa[:3] @ qb[:3]
    v = qa[3] * qb[:3] + qb[3] * qa[:3] + np.cross(qa[:3], qb[:3])
    return np.concatenate([v, [w], a[7] * rot(qa, b[4:7]) + a[4:7], [a[7] * b[7]]])


def path_edges(n):
    return [(i, i - 1, 0) for i in range(1, n)]


def make(seed, nv, edges, fixed=(0,), fix_scale=False, rot_noise=0.02, t_noise=0.05, s_noise=0.02, npoints=0, ref=None,
         scale_spread=0.0, with_nc=True):
    rng = np.random.default_rng(seed)
    truth = np.stack([sim3_row(rng.normal(0, 0.4, 3), rng.normal(0, 2.0, 3), 1.0 if fix_scale else np.exp(rng.normal(0, scale_spread)))
                      for _ in range(nv)]) if nv else np.zeros((0, 8))
    start = np.stack([compose(sim3_row(rng.normal(0, rot_noise, 3), rng.normal(0, t_noise, 3),
                                       1.0 if fix_scale else np.exp(rng.normal(0, s_noise))), truth[v]) for v in range(nv)]) if nv else truth
    fx = np.zeros(nv, np.uint8)
    for v in fixed:
        fx[v] = 1
        start[v] = truth[v]
    p = dict(Scw=start, fixed=fx, edges=np.array(edges, np.int32).reshape(-1, 3), fix_scale=fix_scale)
    if with_nc:
        p["non_corrected"], p["has_non_corrected"] = truth, np.ones(nv, np.uint8)
    p["world"] = rng.normal(0, 3.0, (npoints, 3)).astype(np.float32)
    p["ref"] = np.asarray(rng.integers(0, max(nv, 1), npoints) if ref is None else ref, np.int32)
    return p


def star(seed, nleaves, **kw):
    """hub 0 (free) with nleaves edges; leaf 1 is fixed"""
    return make(seed, nleaves + 1, [(v, 0, 0) for v in range(1, nleaves + 1)], fixed=(1,), **kw)


def cycle_chord(seed, **kw):
    """a fixed vertex 0 hanging on an 8-cycle 1..8 of free vertices with the chord 1-5: eliminating the cycle creates fill"""
    e = [(1, 0, 0)] + [(v + 1, v, 0) for v in range(1, 8)] + [(8, 1, 0), (5, 1, 0)]
    return make(seed, 9, e, **kw)


def consistent():
    """identity rotations, integer translations, scale 1, no NonCorrectedSim3: every product is exact and every error is 0"""
    S = np.array([[0, 0, 0, 1, 3 * v, -v, 2 * v, 1] for v in range(5)], np.float64)
    return dict(Scw=S, fixed=np.array([1, 0, 0, 0, 0], np.uint8), edges=np.array(path_edges(5) + [(4, 0, 1)], np.int32),
                fix_scale=False, world=np.array([[1, 2, 3]], np.float32), ref=np.array([2], np.int32))


def loop(seed=7, n=40, ncorr=6, npoints=257):
    """A drifting circle: the tracked poses drift in scale and heading; the last ncorr keyframes carry a CorrectedSim3 (Scw: the
    drift taken out) and their tracked pose as NonCorrectedSim3; keyframe 0 is pLoopKF (fixed), n - 1 is pCurKF, joined by one
    loop connection.  Edges: spanning tree (i, i - 1), covisibility (i, i - 2), then the loop connection first, as step 3 does."""
    rng = np.random.default_rng(seed)
    true, tracked = [], []
    for i in range(n):
        a = 2 * np.pi * i / n
        Twc = sim3_row([0, 0, a], [5 * np.cos(a), 5 * np.sin(a), 0.1 * np.sin(3 * a)], 1.0)
        q = Twc[:4].copy(); q[:3] = -q[:3]
        Rt = compose(np.concatenate([q, [0, 0, 0, 1.0]]), np.concatenate([[0, 0, 0, 1.0], -Twc[4:7], [1.0]]))
        true.append(Rt)
        drift = sim3_row([0, 0, 0.004 * i] + rng.normal(0, 1e-3, 3), rng.normal(0, 0.01, 3) + [0.01 * i, 0, 0], 1.0)
        d = compose(drift, Rt)
        d[7] = 1.0
        tracked.append(d)
    true, tracked = np.stack(true), np.stack(tracked)
    Scw = tracked.copy()
    has = np.zeros(n, np.uint8)
    for i in range(n - ncorr, n):
        Scw[i] = true[i].copy()
        Scw[i, 7] = 1.0 + 0.02 * (i - (n - ncorr) + 1) / ncorr
        Scw[i, 4:7] *= Scw[i, 7]
        has[i] = 1
    Scw[0] = tracked[0]
    edges = [(n - 1, 0, 1)] + [e for i in range(1, n) for e in ([(i, i - 1, 0)] + ([(i, i - 2, 0)] if i >= 2 else []))]
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    ref = rng.integers(0, n, npoints).astype(np.int32)
    ref[::17] = -1
    ref[1:2] = 0
    return dict(Scw=Scw, fixed=fixed, non_corrected=tracked, has_non_corrected=has, edges=np.array(edges, np.int32), fix_scale=False,
                world=rng.normal(0, 4.0, (npoints, 3)).astype(np.float32), ref=ref)


def chain_covis(seed, n, ncov=3, **kw):
    """the measurement workload: a chain with covisibility edges to the ncov keyframes before the parent"""
    e = [(i, i - k, 0) for i in range(1, n) for k in range(1, ncov + 2) if i - k >= 0]
    return make(seed, n, e, **kw)
