"""compat/Optimizer_localba.inl (the body of Optimizer::LocalBundleAdjustment from :710 on) through the stand-ins of
tests/compat_localba/: built with -Wall -Werror, one small scene run through the fragment on a host-only handle; the poses,
points and erased observations equal the direct orbx_local_bundle_adjustment_batch call (and so tests/localba_model.py).  The
fragment walks std::map<KeyFrame *, size_t>, ascending keyframe address, which is ascending keyframe index in the harness: the
direct call gets every point's observations in that order.  Needs no GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import localba_scenes as sc
from orb_slam2_detailed_comments_amd import ORBextractor, _capi, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "compat_localba")
LIBDIR = os.path.dirname(_capi.LIB_PATH)


def build_cmd(out):
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", "-ffp-contract=off", "-I" + HERE,
           "-I" + os.path.join(ROOT, "tests", "compat_runtime"), "-I" + os.path.join(ROOT, "compat"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "harness.cpp")]
    if out is None:
        return cmd + ["-fsyntax-only"]
    return cmd + ["-shared", "-fPIC", "-L" + LIBDIR, "-lorbx", "-Wl,-rpath," + LIBDIR, "-o", out]


def test_compat_localba_syntax():
    assert shutil.which("g++")
    p = subprocess.run(build_cmd(None), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]


def in_map_order(p):
    """every point's observations in ascending keyframe index"""
    pt = np.repeat(np.arange(len(p["world"])), np.diff(p["obs_begin"]))
    order = np.lexsort((p["obs_kf"], pt))
    q = dict(p)
    for k in ("obs_kf", "obs", "inv_sigma2", "planted", "gross"):
        q[k] = np.ascontiguousarray(p[k][order])
    return q


def run_fragment(L, p, stop=0, bad_point=-1):
    nl, nkf, npt, nobs = p["nlocal"], len(p["Tcw"]), len(p["world"]), len(p["obs_kf"])
    T, w, e = np.full((nl, 16), 7.5, np.float32), np.full((npt, 3), 7.5, np.float32), np.full(nobs, 9, np.uint8)
    info = np.zeros(3, np.int32)
    a = [np.ascontiguousarray(p[k], t) for k, t in (("Tcw", np.float32), ("local_fixed", np.uint8), ("camera", np.float32),
                                                   ("world", np.float32), ("obs_begin", np.int32), ("obs_kf", np.int32),
                                                   ("obs", np.float32), ("inv_sigma2", np.float32))]
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    L.lba_compat_run.restype = C.c_int
    L.lba_compat_run.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_float] + [C.c_void_p] * 5 + [C.c_int] * 2 + [C.c_void_p] * 4
    n = L.lba_compat_run(nl, nkf - nl, npt, ptr(a[0]), ptr(a[1]), ptr(a[2]), float(p["bf"]), ptr(a[3]), ptr(a[4]), ptr(a[5]),
                         ptr(a[6]), ptr(a[7]), stop, bad_point, ptr(T), ptr(w), ptr(e), ptr(info))
    return n, T, w, e, info


def test_fragment_equals_the_direct_call(built_lib, tmp_path):
    so = str(tmp_path / "compat_localba.so")
    b = subprocess.run(build_cmd(so), capture_output=True, text=True, timeout=600)
    assert b.returncode == 0 and "warning" not in b.stderr, b.stderr[-4000:]
    L = C.CDLL(so)
    host = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    try:
        p = in_map_order(sc.make(111, 4, 3, 60, noise=0.7, outlier_frac=0.15, local_fixed=(2,)))
        (T, w, e, info), = optimizer.local_bundle_adjustment_batch(host, [p])
        assert e.sum() > 5
        n, Tf, wf, ef, finfo = run_fragment(L, p)
        assert n == int(e.sum()) and np.array_equal(ef, e)
        assert np.array_equal(Tf.view(np.uint32), T.view(np.uint32)) and np.array_equal(wf.view(np.uint32), w.view(np.uint32))
        assert list(finfo) == [4, 60, 2]                       # SetPose on every local keyframe, the fixed one too; one refresh
        # a point gone bad: its erase entries are dropped, everything else stands
        pt = np.repeat(np.arange(60), np.diff(p["obs_begin"]))
        bad = int(pt[np.nonzero(e)[0][0]])
        n2, T2, w2, e2, _ = run_fragment(L, p, bad_point=bad)
        assert np.array_equal(e2, np.where(pt == bad, 0, e)) and n2 == int(e2.sum()) < n
        assert np.array_equal(T2, Tf) and np.array_equal(w2, wf)
        # the stop flag set on entry: nothing happens
        n3, T3, w3, e3, info3 = run_fragment(L, p, stop=1)
        assert n3 == 0 and list(info3) == [0, 0, 0] and np.array_equal(T3, p["Tcw"][:4]) and np.array_equal(w3, p["world"])
    finally:
        host.close()
