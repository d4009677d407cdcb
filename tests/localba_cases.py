"""The scene lists of tests/test_localba_cpu.py and tests/test_localba_gpu.py with the model's answers, computed once per
process: both files run the same problems and compare with the same function."""
import functools

import numpy as np

import localba_model as lm
import localba_scenes as sc
from orb_slam2_detailed_comments_amd import optimizer

NOISY = dict(noise=0.7, outlier_frac=0.1)
# (seed, nlocal, nfixed, npoints, kwargs).  What the implementation branches on, not the workload: 64 chains over a keyframe's
# edges, over the points and over the free keyframes; 256 lanes over the items of a phase; 0 / 1 / several free keyframes.
SIZES = (
    (1, 1, 0, 1, {}), (2, 1, 1, 63, NOISY), (3, 2, 0, 64, NOISY), (4, 2, 5, 65, NOISY), (5, 3, 1, 257, NOISY), (6, 3, 5, 63, NOISY),
    (7, 12, 5, 257, dict(noise=0.7, outlier_frac=0.2)), (8, 66, 2, 40, dict(noise=0.5, max_obs=6, second_round=False)),
    (9, 3, 2, 140, dict(full_kf=(0, 63), **NOISY)), (10, 3, 2, 140, dict(full_kf=(1, 64), **NOISY)),
    (11, 3, 2, 140, dict(full_kf=(2, 65), **NOISY)), (12, 3, 2, 140, dict(full_kf=(0, 129), **NOISY)),
    (13, 4, 1, 30, dict(mode="mono", **NOISY)), (14, 4, 1, 30, dict(mode="stereo", **NOISY)),
)


def _only(p, which):
    """point 0 keeps its fixed keyframes only, point 1 its free ones only (which = "split"); keyframe 1 loses every edge
    (which = "bare")"""
    pt = np.repeat(np.arange(len(p["world"])), np.diff(p["obs_begin"]))
    local = p["obs_kf"] < p["nlocal"]
    if which == "split":
        return sc.keep_obs(p, ~((pt == 0) & local) & ~((pt == 1) & ~local))
    return sc.keep_obs(p, p["obs_kf"] != 1)


@functools.lru_cache(maxsize=None)
def size_scenes():
    return tuple(sc.make(seed, nl, nf, npt, **kw) for seed, nl, nf, npt, kw in SIZES)


# seeds found by searching with the model alone (the trace says why each one is here)
DEPTH_SEEDS = (118, 121)   # a monocular point started metres off ends behind a keyframe with a small error there
BIG_START = dict(mode="mono", noise=0.5, perturb=(0.1, 0.05, 6.0), max_obs=2)


@functools.lru_cache(maxsize=None)
def special_scenes():
    s = {}
    s["local_fixed"] = sc.make(21, 4, 1, 50, local_fixed=(1,), **NOISY)
    s["all_local_fixed"] = sc.make(22, 2, 1, 20, local_fixed=(0, 1), **NOISY)
    s["split"] = _only(sc.make(23, 3, 3, 40, min_obs=6, **NOISY), "split")
    s["gauge_free"] = sc.make(24, 4, 0, 80, **NOISY)
    s["one_round"] = sc.make(25, 3, 2, 60, second_round=False, **NOISY)
    s["no_points"] = sc.make(26, 2, 1, 0)
    s["no_keyframes"] = sc.make(27, 0, 0, 5)
    for seed in DEPTH_SEEDS:
        s["depth_%d" % seed] = sc.make(seed, 3, 2, 40, **BIG_START)
    return s


@functools.lru_cache(maxsize=None)
def outside_scenes():
    """outside the contract: the same bounded loops run"""
    s = {}
    p = sc.make(31, 2, 2, 30, **NOISY)
    p["Tcw"] = p["Tcw"].copy(); p["world"] = p["world"].copy()
    p["Tcw"][2] = np.eye(4, dtype=np.float32).reshape(16)       # a fixed keyframe at the origin ...
    p["world"][int(np.repeat(np.arange(30), np.diff(p["obs_begin"]))[np.nonzero(p["obs_kf"] == 2)[0][0]])] = (1.0, 1.0, 0.0)   # ... and a point of its at z = 0
    s["z0"] = p
    p = sc.make(32, 2, 2, 30, **NOISY)
    p["world"] = p["world"].copy(); p["world"][3, 1] = np.nan
    s["nan_point"] = p
    p = sc.make(33, 2, 2, 30, **NOISY)
    p["obs"] = p["obs"].copy(); p["obs"][5, 0] = np.inf
    s["inf_obs"] = p
    p = sc.make(34, 3, 1, 30, **NOISY)
    p["Tcw"] = p["Tcw"].copy(); p["Tcw"][0, 3] = np.nan
    s["nan_pose"] = p
    s["bare_keyframe"] = _only(sc.make(35, 3, 2, 40, **NOISY), "bare")
    return s


_MODELS = {}


def model(p):
    """the model's answer and trace for a scene object, computed once"""
    k = id(p)
    if k not in _MODELS:
        tr = []
        _MODELS[k] = (lm.run(p, tr), tr, p)
    return _MODELS[k][0], _MODELS[k][1]


def run(ex, scenes, per_call=16):
    out = []
    for i in range(0, len(scenes), per_call):
        out += optimizer.local_bundle_adjustment_batch(ex, list(scenes[i:i + per_call]))
    return out


def assert_equal(got, mo, what):
    T, w, e, info = got
    assert np.array_equal(T.reshape(-1).view(np.uint32), mo["Tcw"].reshape(-1).view(np.uint32)), what + ": poses"
    assert np.array_equal(w.reshape(-1).view(np.uint32), mo["world"].reshape(-1).view(np.uint32)), what + ": points"
    assert np.array_equal(e, mo["erase"]), what + ": erase"
    assert list(info["iters"]) == list(mo["iters"]), what + ": iterations"
    assert int(info["nerase"]) == mo["nerase"] and int(info["nflagged"]) == mo["nflagged"], what + ": counts"
    assert np.array_equal(np.asarray(info["chi2"]).view(np.uint64), mo["chi2"].view(np.uint64)), what + ": chi2"


def assert_all(ex, named):
    names = list(named)
    got = run(ex, [named[n] for n in names])
    for n, g in zip(names, got):
        assert_equal(g, model(named[n])[0], str(n))


def debug_cases():
    """(problem, est, last) for the classification alone: the estimates after the model's run, "last" = the start estimates and
    the other way round; and a monocular point mirrored behind its keyframe, where the depth test alone decides"""
    out = []
    for p in (size_scenes()[3], size_scenes()[5], special_scenes()["depth_118"]):
        mo = model(p)[0]
        Tend = p["Tcw"].copy(); Tend[:p["nlocal"]] = mo["Tcw"]
        out.append((p, (Tend, mo["world"]), (p["Tcw"], p["world"])))
        out.append((p, (p["Tcw"], p["world"]), (Tend, mo["world"])))
    p = sc.make(41, 1, 1, 6, mode="mono")
    est_world = p["world_true"].copy()
    T = p["Tcw_true"][0].reshape(4, 4).astype(np.float64)
    c = -T[:3, :3].T @ T[:3, 3]
    est_world[0] = (2 * c - est_world[0].astype(np.float64)).astype(np.float32)      # mirrored through keyframe 0's centre
    out.append((p, (p["Tcw_true"], est_world), (p["Tcw_true"], p["world_true"])))
    return out
