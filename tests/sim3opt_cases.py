"""What tests/test_sim3opt_cpu.py and tests/test_sim3opt_gpu.py share: the size list, the committed branch seeds, the scenes
outside the contract, the model's answers (computed once per process and never changed) and the exact comparison."""
import functools

import numpy as np

import sim3opt_model as sm
import sim3opt_scenes as ss
from orb_slam2_detailed_comments_amd import optimizer

# the < 10 return, the caller's 20, both sides of a 64-lane chunk and of two chunks
SIZES = (0, 1, 9, 10, 11, 19, 20, 63, 64, 65, 129)
# (seed, n, fix_scale, noise, outlier_frac, rot_deg, trans, scale_pct): found by search over the model's trace on the CPU
BRANCH_SEEDS = (
    (0, 30, 0, 1.0, 0.2, 3, 0.05, 3),        # nBad > 0 -> 10 more iterations; a rejected trial; the three-stall stop
    (0, 40, 1, 0.5, 0.0, 3, 0.05, 3),        # nBad == 0 -> 5 more iterations, fix_scale
    (0, 14, 0, 1.0, 0.2, 3, 0.05, 3),        # the early return 0 with first-stage nulls
    (1, 40, 1, 0.5, 0.0, 3, 0.05, 3),        # rho == 0
    (9, 40, 1, 0.5, 0.0, 3, 0.05, 3),        # ten rejections in a row (Terminate)
    (12, 50, 0, 0.3, 0.0, 25, 1.0, 40),      # ten rejections, free scale, a start far off
)
RESULT_FIELDS = ("r", "t", "s", "T12", "ninliers", "nbad", "ncorr", "written")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def model(s, trace=None):
    return sm.optimize_sim3(s, trace)


@functools.lru_cache(maxsize=None)
def size_scenes():
    """the size list with fix_scale 0 and 1: below 19 no planted outliers, so that 10 and 11 go on to the second optimisation"""
    scenes = [ss.make(100 + n, n, fs, noise=0.5, outlier_frac=0.1 if n >= 19 else 0.0) for n in SIZES for fs in (0, 1)]
    return scenes, [model(s) for s in scenes]


@functools.lru_cache(maxsize=None)
def branch_scenes():
    scenes, models, traces = [], [], []
    for seed, n, fs, noise, of, rot, tr, sp in BRANCH_SEEDS:
        s = ss.make(seed, n, fs, noise=noise, outlier_frac=of, rot_deg=rot, trans=tr, scale_pct=sp)
        t = {}
        scenes.append(s)
        models.append(model(s, t))
        traces.append(t)
    return scenes, models, traces


@functools.lru_cache(maxsize=None)
def special_scenes():
    """outside the contract: (name, scene)"""
    out = []
    base = ss.make(4, 30, 0, noise=1.0, outlier_frac=0.1)
    for name, poison in (("inf", (np.inf, 1.0, 2.0)), ("nan", (np.nan, np.nan, np.nan)), ("1e30", (1e30, -1e30, 1e-30))):
        x2 = base["x2c"].copy()
        x2[:3] = poison
        x1 = base["x1c"].copy()
        x1[5] = poison
        out.append((name, ss.variant(base, x1c=x1, x2c=x2)))
    # a point at z = 0 after map: identity start, x2c[0].z = 0 exactly, t.z = 0
    s = ss.make(3, 40, 0, noise=1.0, outlier_frac=0.2)
    x2 = s["x2c"].copy()
    x2[0] = (0.5, -0.25, 0.0)
    out.append(("z = 0", ss.variant(s, x2c=x2, R=np.eye(3, dtype=np.float32), t=np.zeros(3, np.float32), s=np.float32(1))))
    out.append(("s = 0", ss.variant(base, s=np.float32(0))))
    out.append(("s = 0, fixed", ss.variant(base, s=np.float32(0), fix_scale=1)))
    out.append(("s = nan", ss.variant(base, s=np.float32(np.nan))))
    out.append(("zero information", ss.variant(base, inv_sigma2_1=np.zeros(30, np.float32), inv_sigma2_2=np.zeros(30, np.float32))))
    obs = base["obs1"].copy()
    obs[7] = (np.nan, np.inf)
    out.append(("obs nan", ss.variant(base, obs1=obs)))
    out.append(("th2 nan", ss.variant(base, th2=np.float32(np.nan))))
    return out


def run(ex, scenes, results=None):
    """one orbx_optimize_sim3_batch call -> (results, keep rows as prefilled by sim3opt_scenes.problem)"""
    return optimizer.optimize_sim3_batch(ex, [ss.problem(s) for s in scenes], results)


def assert_same(res, keep, want, s, what):
    wres, wkeep = want
    n = s["n"]
    for f in RESULT_FIELDS:
        a = np.asarray(res[f])
        b = np.asarray(wres[f], a.dtype).reshape(a.shape)
        assert a.tobytes() == b.tobytes(), (what, f, a, b)
    assert np.array_equal(keep[:n], wkeep), (what, "keep")
    assert (keep[n:] == ss.PREFILL_KEEP).all(), (what, "keep bytes past n")


def assert_all(got, scenes, models, what):
    results, keeps = got
    for k, (s, m) in enumerate(zip(scenes, models)):
        assert_same(results[k], keeps[k], m, s, f"{what}, problem {k} (n = {s['n']})")
        nkept = int(np.count_nonzero(keeps[k][:s["n"]]))
        assert int(results[k]["ninliers"]) == (nkept if int(results[k]["written"]) else 0), what


@functools.lru_cache(maxsize=None)
def stale_case():
    """a scene, the estimate and a `last` a few centimetres off: the chi2 test at `last` gives other flags than at the estimate"""
    s = ss.make(21, 80, 0, noise=1.5, outlier_frac=0.1)
    tr = {}
    model(s, tr)
    est = tr["stages"][0]["est"]
    q, t, sc = est
    last = (q, (t[0] + np.float64(0.03), t[1] - np.float64(0.02), t[2] + np.float64(0.04)), sc * np.float64(1.01))
    return s, sm.sim3_as8(est), sm.sim3_as8(last)


def run_inlier_test(ex, s, S_last):
    return optimizer.debug_sim3opt_inlier_test(ex, [ss.problem(s)], [S_last])


def assert_inlier_test(got, s, est8, last8):
    results, keeps = got
    want = sm.inlier_test(s, last8)
    at_est = sm.inlier_test(s, est8)
    assert not np.array_equal(want[1], at_est[1])                        # the scene tells "at the last trial" from "at the estimate"
    assert_same(results[0], keeps[0], want, s, "inlier test at the last trial's Sim3")
