"""The Levenberg-Marquardt core shared by PoseOptimization and OptimizeSim3 (csrc/orbx_lm.h, tests/lm_model.py) against results
recorded BEFORE the two copies were merged: tests/golden/lm_parent_pin.npz holds, for the size lists, the branch seeds and the
scenes outside the contract of both optimizers, what the models and the library's host path gave at the commit named in
tests/golden/README.md (they agreed there), and per scene the number of LM iterations and trials of the model's trace.  Model and
code changed in one commit, so "device = host = model" alone could not see an error made the same way in both; this can.  Needs no
GPU.  `PYTHONPATH=. python tests/test_lm_parent_pin.py --write` (from the repository's root, library built) records the fixture anew (only ever at a commit whose results are to be kept)."""
import os
import sys

import numpy as np
import pytest

import pose_cases
import pose_scenes as ps
import sim3opt_cases
from orb_slam2_detailed_comments_amd import ORBextractor, _capi

PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_parent_pin.npz")


def pose_scenes():
    """(name, scene, model kwargs): sizes, branch seeds, the special scenes and the scenes outside the contract of
    test_pose_batch_cpu.py (a point at z = 0 of the start pose, non-finite and extreme points)"""
    out = [(f"size {s['nfeat']}/{k}", s, {}) for k, s in enumerate(pose_cases.size_scenes()[0])]
    out += [(f"branch {seed}", s, {}) for s, (seed, _, _) in zip(pose_cases.branch_scenes()[0], pose_cases.BRANCH_SEEDS)]
    out += pose_cases.special_scenes()
    s = ps.make(3, 40, "mono", noise=1.0, outlier_frac=0.2)
    T0 = np.eye(4, dtype=np.float32)
    T0[:3, 3] = (0.25, -0.125, 0.5)
    world = s["world"].copy()
    world[s["point"][s["point"] >= 0][0]] = (1.0, 2.0, -0.5)
    out.append(("z = 0", ps.variant(s, Tcw0=T0, world=world), {}))
    for poison in ((np.inf, 1.0, 2.0), (np.nan, np.nan, np.nan), (1e30, -1e30, 1e-30), (0.0, 0.0, 0.0)):
        s = ps.make(4, 30, "mixed", noise=1.0)
        world = s["world"].copy()
        world[s["point"][s["point"] >= 0][:3]] = poison
        out.append((f"poison {poison}", ps.variant(s, world=world), {}))
    return out


def sim3_scenes():
    return (list(sim3opt_cases.size_scenes()[0]) + list(sim3opt_cases.branch_scenes()[0])
            + [s for _, s in sim3opt_cases.special_scenes()])


def _counts(groups):
    iters = [i for g in groups for i in g["iters"]]
    return len(iters), sum(len(i["trials"]) for i in iters)


def _pose_bytes(T, outlier, ninliers):
    return np.ascontiguousarray(T, np.float32).tobytes() + np.ascontiguousarray(outlier, np.uint8).tobytes() + np.int32(ninliers).tobytes()


def _sim3_bytes(res, keep, n):
    rec = np.zeros(1, _capi.SIM3OPT_RESULT_DTYPE)
    for f in sim3opt_cases.RESULT_FIELDS:
        rec[0][f] = np.asarray(res[f], rec.dtype[f].base).reshape(rec.dtype[f].shape)
    return rec.tobytes() + np.ascontiguousarray(keep[:n], np.uint8).tobytes()


def collect(host):
    """-> {"pose_model", "pose_host", "sim3_model", "sim3_host": uint8 (all scenes' result bytes, in order),
    "pose_counts", "sim3_counts": int32 [scenes][2] = LM iterations, trials of the model's trace}"""
    pm_, ph_, pc_ = [], [], []
    for name, s, kw in pose_scenes():
        tr = {}
        pm_.append(_pose_bytes(*pose_cases.model(s, trace=tr, **kw)))
        ph_.append(_pose_bytes(*pose_cases.single(host, s, **kw)))
        pc_.append(_counts(tr["rounds"]))
    scenes = sim3_scenes()
    sm_, sc_ = [], []
    for s in scenes:
        tr = {}
        res, keep = sim3opt_cases.model(s, tr)
        sm_.append(_sim3_bytes(res, keep, s["n"]))
        sc_.append(_counts(tr["stages"]))
    results, keeps = sim3opt_cases.run(host, scenes)
    sh_ = [results[k:k + 1].tobytes() + np.ascontiguousarray(keeps[k][:s["n"]], np.uint8).tobytes() for k, s in enumerate(scenes)]
    join = lambda parts: np.frombuffer(b"".join(parts), np.uint8)
    return {"pose_model": join(pm_), "pose_host": join(ph_), "sim3_model": join(sm_), "sim3_host": join(sh_),
            "pose_counts": np.array(pc_, np.int32), "sim3_counts": np.array(sc_, np.int32)}


def test_models_and_host_path_reproduce_the_results_recorded_before_the_merge(built_lib):
    want = np.load(PIN)
    assert np.array_equal(want["pose_model"], want["pose_host"]) and np.array_equal(want["sim3_model"], want["sim3_host"])
    for c in (want["pose_counts"], want["sim3_counts"]):       # the trace was recorded: a scene that iterates makes trials
        assert (c[:, 1] >= c[:, 0]).all() and (c[:, 1] > c[:, 0]).any() and np.count_nonzero(c[:, 0]) >= len(c) - 2
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    try:
        got = collect(ex)
    finally:
        ex.close()
    assert sorted(got) == sorted(want.files)
    for key in sorted(got):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert got[key].tobytes() == want[key].tobytes(), key


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: PYTHONPATH=. python tests/test_lm_parent_pin.py --write")
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    rec = collect(ex)
    ex.close()
    np.savez_compressed(PIN, **rec)
    print({k: (v.shape, int(v.sum())) for k, v in rec.items()}, os.path.getsize(PIN), "bytes")
