"""What tests/test_pose_batch_cpu.py and tests/test_pose_batch_gpu.py share: the committed scenes (size list, branch seeds,
special scenes), the model's answers for them (computed once per process), one call through the Python wrapper over prefilled
rows, and the exact comparisons."""
import ctypes as C

import numpy as np

import pose_model as pm
import pose_scenes as ps
from orb_slam2_detailed_comments_amd import _capi, optimizer

SIZES = (0, 2, 3, 9, 10, 63, 64, 65, 130, 256)
CAP = 256
# committed seeds (searched on the CPU over pose_scenes.make(seed, n, mode, 1.0, 0.2, perturb=(0.1, 0.05)))
BRANCH_SEEDS = ((100, 20, "stereo"), (102, 65, "mono"), (109, 40, "stereo"), (107, 130, "mixed"))
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def model(s, trace=None, **kw):
    a = ps.model_args(s)
    a.update(kw)
    return pm.pose_optimization(trace=trace, **a)


def single(ex, s, **kw):
    a = dict(Tcw=s["Tcw0"], keys_un=s["keys"], u_right=s["u_right"], point=s["point"], world_pos=s["world"], camera4=ps.CAMERA4,
             mbf=ps.MBF, inv_level_sigma2=ps.INV_SIGMA2)
    a.update(kw)
    return optimizer.pose_optimization(ex, **a)


def assert_same(got, want, tag=""):
    (T, o, n), (Tm, om, nm) = got, want
    assert np.array_equal(bits(T), bits(Tm)), f"{tag}: pose differs from the model\n{T}\n{Tm}"
    assert np.array_equal(o, om), f"{tag}: outlier flags differ from the model"
    assert n == nm, f"{tag}: {n} inliers, the model has {nm}"


def size_scenes():
    """the size list, modes in rotation, one pixel of noise and planted outliers; computed once, shared with the GPU tests"""
    if "sizes" not in _CACHE:
        sc = [ps.make(40 + k, n, ("mono", "stereo", "mixed")[k % 3], 1.0, 0.2, nfeat=CAP if n == CAP else None)
              for k, n in enumerate(SIZES)]
        _CACHE["sizes"] = (sc, [model(s) for s in sc])
    return _CACHE["sizes"]


def branch_scenes():
    if "branch" not in _CACHE:
        sc = [ps.make(seed, n, mode, 1.0, 0.2, perturb=(0.1, 0.05)) for seed, n, mode in BRANCH_SEEDS]
        traces = [dict() for _ in sc]
        _CACHE["branch"] = (sc, [model(s, trace=t) for s, t in zip(sc, traces)], traces)
    return _CACHE["branch"]


def special_scenes():
    """(name, scene, model kwargs): a round with no active edge, all points on one ray, zero information (the solve fails)"""
    return [("all-gross", ps.make(11, 30, "mixed", 1.0, 1.0), {}),
            ("ray-mono", ps.ray(12, 20, "mono"), {}),
            ("ray-stereo", ps.ray(12, 20, "stereo"), {}),
            ("zero-information", ps.make(13, 30, "mixed", 1.0, 0.0), dict(inv_level_sigma2=np.zeros(8, np.float32)))]


def run_batch(ex, scenes, cap=CAP, frame_of=None, use_index=True, to_dev=lambda a: a, to_host=lambda a: a, sig=ps.INV_SIGMA2):
    """one call; rows prefilled so that untouched entries show"""
    b = ps.batch(scenes, cap, frame_of, use_index)
    k = max(len(scenes), 1)
    T = to_dev(np.full((k, 16), ps.PREFILL_T, np.float32))
    o = to_dev(np.full((k, cap), ps.PREFILL_OUTLIER, np.uint8))
    n = to_dev(np.full(k, ps.PREFILL_N, np.int32))
    keys = to_dev(b["keys"].view(np.uint8).reshape(b["nframes"], -1))
    optimizer.pose_optimization_batch(ex, b["problems"], b["world"], b["nframes"], keys, to_dev(b["u_right"]), to_dev(b["counts"]),
                                      cap, to_dev(b["point"]), ps.CAMERA4, ps.MBF, sig, T, o, n)
    return to_host(T), to_host(o), to_host(n)


def assert_rows(got, want, tag=""):
    for g, w, what in zip(got, want, ("pose rows", "outlier rows", "inlier counts")):
        g, w = np.asarray(g), np.asarray(w)
        same = np.array_equal(bits(g), bits(w)) if g.dtype == np.float32 else np.array_equal(g, w)
        assert same, f"{tag}: {what} differ from the model\n{g}\n{w}"


def stale_case():
    """a scene for orbx_debug_pose_inlier_test: the estimate is the true pose, the pose of the last (rejected) trial the perturbed
    start pose, a few centimetres and a degree away -- far enough for many decisions to depend on which pose an edge is tested at;
    the flags on entry are a random half.  -> (scene, est, last, flags, the model's (flags, ninliers))"""
    if "stale" not in _CACHE:
        s = ps.make(21, 120, "mixed", noise=1.0, outlier_frac=0.2, perturb=(0.05, 0.03))
        flags = (np.random.default_rng(3).random(s["nfeat"]) < 0.5).astype(np.uint8)
        a = ps.model_args(s)
        a.pop("Tcw")
        _CACHE["stale"] = (s, s["Tcw_true"], s["Tcw0"], flags, a)
    s, est, last, flags, a = _CACHE["stale"]
    return s, est, last, flags, pm.inlier_test(est, last, flags, **a)


def run_inlier_test(ex, s, est, last, flags, cap=CAP, to_dev=lambda a: a, to_host=lambda a: a):
    """orbx_debug_pose_inlier_test for one problem; the outlier row is prefilled, then the flags are laid over the frame's features"""
    b = ps.batch([s], cap)
    row = np.full((1, cap), ps.PREFILL_OUTLIER, np.uint8)
    has = s["point"] >= 0
    row[0, :s["nfeat"]][has] = flags[has]
    o, n = to_dev(row), to_dev(np.full(1, ps.PREFILL_N, np.int32))
    prob = (_capi.PoseProblem * 1)()
    idx = np.ascontiguousarray(b["problems"][0]["point_index"], np.int32)
    prob[0].frame, prob[0].npoints, prob[0].point_index = 0, len(idx), idx.ctypes.data
    prob[0].Tcw[:] = np.asarray(s["Tcw0"], np.float32).reshape(16).tolist()
    P = _capi.ptr
    e16, l16 = np.ascontiguousarray(est, np.float32).reshape(16), np.ascontiguousarray(last, np.float32).reshape(16)
    world = np.ascontiguousarray(b["world"], np.float32)
    keys, ur, cnt, pt = (to_dev(x) for x in (b["keys"].view(np.uint8).reshape(1, -1), b["u_right"], b["counts"], b["point"]))   # kept alive
    _capi.check(_capi.lib().orbx_debug_pose_inlier_test(
        ex.handle, 1, C.cast(prob, C.c_void_p), len(world), P(world), 1, P(keys), P(ur), P(cnt), cap, P(pt), P(ps.CAMERA4),
        float(ps.MBF), P(ps.INV_SIGMA2), len(ps.INV_SIGMA2), P(e16), P(l16), P(o), P(n)))
    got = to_host(o)[0], int(to_host(n)[0])
    del keys, ur, cnt, pt
    return got


def assert_inlier_test(got, s, est, last, flags, want):
    """the library's flags equal the model's, and the model's differ from both one-pose rules (so the test tells them apart)"""
    a = ps.model_args(s)
    a.pop("Tcw")
    row, n = got
    nf, has = s["nfeat"], s["point"] >= 0
    assert np.array_equal(row[:nf][has], want[0][has]) and n == want[1], "inlier test differs from the model"
    assert (row[:nf][~has] == ps.PREFILL_OUTLIER).all() and (row[nf:] == ps.PREFILL_OUTLIER).all()
    for one in (est, last):
        other = pm.inlier_test(one, one, flags, **a)
        assert not np.array_equal(other[0][has], want[0][has]), "the scene does not tell the rules apart"
