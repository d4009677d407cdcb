"""Optimizer::PoseOptimization(Frame*) for tracked frames (include/orbx.h: orbx_pose_optimization_batch_device,
orbx_pose_optimization), Optimizer::OptimizeSim3 for loop-closure candidates (orbx_optimize_sim3_batch) Optimizer::LocalBundleAdjustment for local mapping (orbx_local_bundle_adjustment_batch) and Optimizer::OptimizeEssentialGraph for loop closing (orbx_optimize_essential_graph_batch).  ctypes marshalling only; `extractor` is the ORBextractor whose handle (stream, staging block) the
calls run on.  The batch reads the frames where the device batch left them and writes poses, outlier rows and inlier counts on
the device; nothing is downloaded.  On a host-only extractor (device=-2) every device argument is a numpy array and the
library's host path runs."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, ptr


def pose_optimization_batch(extractor, problems, world_pos, nframes, d_keys_un, d_u_right, d_counts, cap, d_point, camera4, mbf,
                            inv_level_sigma2, d_Tcw, d_outlier, d_ninliers):
    """problems: dicts with frame, Tcw (4x4), optionally point_index (list position -> pool index) and npoints (default: the
    length of point_index, or the pool's size).  d_point [nproblems, cap] int32: -1 or the list position of the feature's
    MapPoint -- a d_assigned row of the map-point / local-point matchers as it stands.  d_Tcw [nproblems, 16] float32,
    d_outlier [nproblems, cap] uint8, d_ninliers [nproblems] int32 are written on the device, asynchronously."""
    world = np.ascontiguousarray(world_pos, np.float32).reshape(-1, 3)
    cam = np.ascontiguousarray(camera4, np.float32)
    sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
    arr = (_capi.PoseProblem * max(len(problems), 1))()
    keep = []
    for k, p in enumerate(problems):
        arr[k].frame = int(p["frame"])
        arr[k].Tcw[:] = np.asarray(p["Tcw"], np.float32).reshape(16).tolist()
        idx = p.get("point_index")
        if idx is not None:
            idx = np.ascontiguousarray(idx, np.int32)
            keep.append(idx)
            arr[k].point_index = idx.ctypes.data if idx.size else None
        arr[k].npoints = int(p.get("npoints", len(idx) if idx is not None else len(world)))
    check(_capi.lib().orbx_pose_optimization_batch_device(
        extractor.handle, len(problems), C.cast(arr, C.c_void_p), len(world), ptr(world) if world.size else None, int(nframes),
        ptr(d_keys_un), ptr(d_u_right), ptr(d_counts), int(cap), ptr(d_point), ptr(cam), float(mbf), ptr(sig), len(sig),
        ptr(d_Tcw), ptr(d_outlier), ptr(d_ninliers)))
    return d_Tcw, d_outlier, d_ninliers


def pose_optimization(extractor, Tcw, keys_un, u_right, point, world_pos, camera4, mbf, inv_level_sigma2, outlier=None):
    """One frame on the host: keys_un [n] KP_DTYPE, u_right [n] or None (all monocular), point [n] = -1 or the pool index of the
    feature's MapPoint.  Returns (Tcw 4x4 float32, outlier uint8 [n], ninliers); with fewer than 3 correspondences the pose comes
    back as it went in and ninliers is 0."""
    keys = np.ascontiguousarray(keys_un, _capi.KP_DTYPE)
    n = len(keys)
    ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
    pt = np.ascontiguousarray(point, np.int32)
    world = np.ascontiguousarray(world_pos, np.float32).reshape(-1, 3)
    cam = np.ascontiguousarray(camera4, np.float32)
    sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
    T = np.array(Tcw, np.float32).reshape(4, 4)
    outlier = np.zeros(n, np.uint8) if outlier is None else outlier
    assert outlier.dtype == np.uint8 and outlier.flags.c_contiguous and len(outlier) == n and len(pt) == n
    nin = C.c_int32(0)
    check(_capi.lib().orbx_pose_optimization(extractor.handle, ptr(T), n, ptr(keys), ptr(ur), ptr(pt), len(world),
                                             ptr(world) if world.size else None, ptr(cam), float(mbf), ptr(sig), len(sig),
                                             ptr(outlier), C.byref(nin)))
    return T, outlier, int(nin.value)


def _sim3opt_marshal(problems):
    arr = (_capi.Sim3OptProblem * max(len(problems), 1))()
    hold, keeps = [], []
    for k, p in enumerate(problems):
        x1 = np.ascontiguousarray(p["x1c"], np.float32).reshape(-1, 3)
        x2 = np.ascontiguousarray(p["x2c"], np.float32).reshape(-1, 3)
        o1 = np.ascontiguousarray(p["obs1"], np.float32).reshape(-1, 2)
        o2 = np.ascontiguousarray(p["obs2"], np.float32).reshape(-1, 2)
        w1 = np.ascontiguousarray(p["inv_sigma2_1"], np.float32).reshape(-1)
        w2 = np.ascontiguousarray(p["inv_sigma2_2"], np.float32).reshape(-1)
        n = len(x1)
        assert len(x2) == n and len(o1) == n and len(o2) == n and len(w1) == n and len(w2) == n
        keep = p.get("keep")
        if keep is None:
            keep = np.zeros(n, np.uint8)
        assert keep.dtype == np.uint8 and keep.flags.c_contiguous and len(keep) >= n
        hold += [x1, x2, o1, o2, w1, w2]
        keeps.append(keep)
        a = arr[k]
        a.n = n
        a.x1c, a.x2c, a.obs1, a.obs2, a.inv_sigma2_1, a.inv_sigma2_2 = (v.ctypes.data if n else None for v in (x1, x2, o1, o2, w1, w2))
        a.keep = keep.ctypes.data if n else None
        a.camera1[:] = np.asarray(p["camera1"], np.float32).tolist()
        a.camera2[:] = np.asarray(p["camera2"], np.float32).tolist()
        a.R[:] = np.asarray(p["R"], np.float32).reshape(9).tolist()
        a.t[:] = np.asarray(p["t"], np.float32).reshape(3).tolist()
        a.s = float(np.float32(p["s"]))
        a.th2 = float(np.float32(p["th2"]))
        a.fix_scale = int(bool(p["fix_scale"]))
    return arr, hold, keeps


def optimize_sim3_batch(extractor, problems, results=None):
    """Optimizer::OptimizeSim3 for many (candidate, matches, Sim3) problems in one call.  problems: dicts with x1c, x2c [n, 3]
    (P3D1c, P3D2c of the correspondences that passed OptimizeSim3's own filters, in order of i), obs1, obs2 [n, 2], inv_sigma2_1,
    inv_sigma2_2 [n], camera1, camera2 (fx, fy, cx, cy), R [3, 3], t [3], s (the solver's estimate), th2, fix_scale and optionally
    keep (uint8, at least n entries, written in place).  Returns (results, keeps): results a record array of
    _capi.SIM3OPT_RESULT_DTYPE (r, t, s = g2oS12 on return, T12, ninliers, nbad, ncorr, written), keeps[k] uint8 with 1 where
    vpMatches1[idx] survives.  On a host-only extractor the library's host path runs."""
    arr, hold, keeps = _sim3opt_marshal(problems)
    if results is None:
        results = np.zeros(len(problems), _capi.SIM3OPT_RESULT_DTYPE)
    assert results.dtype == _capi.SIM3OPT_RESULT_DTYPE and results.flags.c_contiguous and len(results) >= len(problems)
    check(_capi.lib().orbx_optimize_sim3_batch(extractor.handle, len(problems), C.cast(arr, C.c_void_p),
                                               ptr(results) if len(problems) else None))
    return results, keeps


def debug_sim3opt_inlier_test(extractor, problems, S_last):
    """parity tests only (orbx_debug_sim3opt_inlier_test): S_last [nproblems, 8] float64 = r x y z w, t, s"""
    arr, hold, keeps = _sim3opt_marshal(problems)
    last = np.ascontiguousarray(S_last, np.float64).reshape(-1, 8)
    assert len(last) == len(problems)
    results = np.zeros(len(problems), _capi.SIM3OPT_RESULT_DTYPE)
    check(_capi.lib().orbx_debug_sim3opt_inlier_test(extractor.handle, len(problems), C.cast(arr, C.c_void_p), ptr(last),
                                                     ptr(results)))
    return results, keeps


def _localba_marshal(problems, debug=False):
    arr = (_capi.LocalBAProblem * max(len(problems), 1))()
    hold, outs = [], []
    for k, p in enumerate(problems):
        T = np.ascontiguousarray(p["Tcw"], np.float32).reshape(-1, 16)
        nlocal = int(p["nlocal"])
        lf = np.ascontiguousarray(p.get("local_fixed", np.zeros(nlocal, np.uint8)), np.uint8).reshape(-1)
        world = np.ascontiguousarray(p["world"], np.float32).reshape(-1, 3)
        begin = np.ascontiguousarray(p["obs_begin"], np.int32).reshape(-1)
        kf = np.ascontiguousarray(p["obs_kf"], np.int32).reshape(-1)
        obs = np.ascontiguousarray(p["obs"], np.float32).reshape(-1, 3)
        w = np.ascontiguousarray(p["inv_sigma2"], np.float32).reshape(-1)
        nobs = len(kf)
        assert len(lf) == nlocal and len(T) >= nlocal and len(begin) == len(world) + 1 and len(obs) == nobs and len(w) == nobs
        Tout = p.get("Tcw_out")
        Tout = np.zeros((nlocal, 16), np.float32) if Tout is None else Tout
        wout = p.get("world_out")
        wout = np.zeros((len(world), 3), np.float32) if wout is None else wout
        erase = p.get("erase")
        erase = np.zeros(nobs, np.uint8) if erase is None else erase
        assert Tout.dtype == np.float32 and Tout.flags.c_contiguous and Tout.size == 16 * nlocal
        assert wout.dtype == np.float32 and wout.flags.c_contiguous and wout.size == 3 * len(world)
        assert erase.dtype == np.uint8 and erase.flags.c_contiguous and erase.size == nobs
        hold += [T, lf, world, begin, kf, obs, w]
        outs.append((Tout, wout, erase))
        a = arr[k]
        a.nlocal, a.nfixed, a.npoints = nlocal, len(T) - nlocal, len(world)
        a.second_round = int(bool(p.get("second_round", True)))
        a.Tcw = T.ctypes.data if len(T) else None
        a.local_fixed = lf.ctypes.data if nlocal else None
        a.camera[:] = np.asarray(p["camera"], np.float32).tolist()
        a.bf = float(np.float32(p["bf"]))
        a.world = world.ctypes.data if len(world) else None
        a.obs_begin = begin.ctypes.data
        a.obs_kf, a.obs, a.inv_sigma2 = (v.ctypes.data if nobs else None for v in (kf, obs, w))
        a.Tcw_out = Tout.ctypes.data if nlocal else None
        a.world_out = wout.ctypes.data if len(world) else None
        a.erase = erase.ctypes.data if nobs else None
    return arr, hold, outs


def local_bundle_adjustment_batch(extractor, problems):
    """Optimizer::LocalBundleAdjustment for many local maps in one call (orbx_local_bundle_adjustment_batch).  problems: dicts
    with nlocal, Tcw [nlocal + nfixed, 16] (the local keyframes in list order, then the fixed ones), optionally local_fixed
    [nlocal] uint8 (mnId == 0), camera (fx, fy, cx, cy), bf, world [npoints, 3], obs_begin [npoints + 1] (CSR by point), obs_kf
    [nobs], obs [nobs, 3] (x, y, mvuRight; < 0: monocular), inv_sigma2 [nobs], second_round (default True: what bDoMore would be)
    and optionally Tcw_out / world_out / erase to be written in place.  Returns per problem (Tcw [nlocal, 16] float32, world
    [npoints, 3] float32, erase [nobs] uint8, info), info a record of _capi.LOCALBA_RESULT_DTYPE (iters, nflagged, nerase, chi2).
    On a host-only extractor the library's host path runs."""
    arr, hold, outs = _localba_marshal(problems)
    results = np.zeros(len(problems), _capi.LOCALBA_RESULT_DTYPE)
    check(_capi.lib().orbx_local_bundle_adjustment_batch(extractor.handle, len(problems), C.cast(arr, C.c_void_p),
                                                         ptr(results) if len(problems) else None))
    return [(T, w, e, results[k]) for k, (T, w, e) in enumerate(outs)]


def debug_localba_classify(extractor, problems, states):
    """parity tests only (orbx_debug_localba_classify): states[k] = (Tcw_est, world_est, Tcw_last, world_last), float32 arrays
    shaped like the problem's Tcw and world.  Returns per problem (erase, info)."""
    arr, hold, outs = _localba_marshal(problems)
    st = (_capi.LocalBADebug * max(len(problems), 1))()
    for k, s in enumerate(states):
        a = [np.ascontiguousarray(v, np.float32) for v in s]
        hold += a
        st[k].Tcw_est, st[k].world_est, st[k].Tcw_last, st[k].world_last = (v.ctypes.data if v.size else None for v in a)
    results = np.zeros(len(problems), _capi.LOCALBA_RESULT_DTYPE)
    check(_capi.lib().orbx_debug_localba_classify(extractor.handle, len(problems), C.cast(arr, C.c_void_p), C.cast(st, C.c_void_p),
                                                  ptr(results) if len(problems) else None))
    return [(e, results[k]) for k, (T, w, e) in enumerate(outs)]


def _essgraph_marshal(problems):
    arr = (_capi.EssGraphProblem * max(len(problems), 1))()
    hold, outs = [], []
    for k, p in enumerate(problems):
        S = np.ascontiguousarray(p["Scw"], np.float64).reshape(-1, 8)
        nv = len(S)
        fixed = np.ascontiguousarray(p.get("fixed", np.zeros(nv, np.uint8)), np.uint8).reshape(-1)
        nc, has = p.get("non_corrected"), p.get("has_non_corrected")
        if nc is not None:
            nc = np.ascontiguousarray(nc, np.float64).reshape(-1, 8)
            has = np.ascontiguousarray(has, np.uint8).reshape(-1)
            assert len(nc) == nv and len(has) == nv
        edges = np.ascontiguousarray(p.get("edges", np.zeros((0, 3), np.int32)), np.int32).reshape(-1, 3)
        world = np.ascontiguousarray(p.get("world", np.zeros((0, 3), np.float32)), np.float32).reshape(-1, 3)
        ref = np.ascontiguousarray(p.get("ref", np.zeros(0, np.int32)), np.int32).reshape(-1)
        assert len(fixed) == nv and len(ref) == len(world)
        Sout, Tout, wout = p.get("Siw_out"), p.get("Tiw_out"), p.get("world_out")
        Sout = np.zeros((nv, 8), np.float64) if Sout is None else Sout
        Tout = np.zeros((nv, 16), np.float32) if Tout is None else Tout
        wout = np.zeros((len(world), 3), np.float32) if wout is None else wout
        assert Sout.dtype == np.float64 and Sout.flags.c_contiguous and Sout.size == 8 * nv
        assert Tout.dtype == np.float32 and Tout.flags.c_contiguous and Tout.size == 16 * nv
        assert wout.dtype == np.float32 and wout.flags.c_contiguous and wout.size == 3 * len(world)
        hold += [S, fixed, nc, has, edges, world, ref]
        outs.append((Sout, Tout, wout))
        a = arr[k]
        a.nvertices, a.nedges, a.npoints, a.fix_scale = nv, len(edges), len(world), int(bool(p.get("fix_scale", False)))
        a.Scw, a.fixed = (v.ctypes.data if nv else None for v in (S, fixed))
        a.non_corrected = nc.ctypes.data if nc is not None and nv else None
        a.has_non_corrected = has.ctypes.data if nc is not None and nv else None
        a.edges = edges.ctypes.data if len(edges) else None
        a.world, a.ref = (v.ctypes.data if len(world) else None for v in (world, ref))
        a.Siw_out, a.Tiw_out = (v.ctypes.data if nv else None for v in (Sout, Tout))
        a.world_out = wout.ctypes.data if len(world) else None
    return arr, hold, outs


def optimize_essential_graph_batch(extractor, problems):
    """Optimizer::OptimizeEssentialGraph for many pose graphs in one call (orbx_optimize_essential_graph_batch).  problems: dicts
    with Scw [nv, 8] float64 (vScw: quaternion x y z w, t, s; loopclosing.sim3_from_Tcw for a keyframe without a CorrectedSim3),
    optionally fixed [nv] uint8 (pKF == pLoopKF), non_corrected [nv, 8] with has_non_corrected [nv] (NonCorrectedSim3), edges
    [ne, 3] int32 (i, j, kind; loopclosing.essential_graph_edges), fix_scale, world [npoints, 3] float32 and ref [npoints] int32
    (the vertex a point is corrected by, -1: a bad point, copied through), and optionally Siw_out / Tiw_out / world_out to be
    written in place.  Returns per problem (Siw [nv, 8] float64, Tiw [nv, 16] float32, world [npoints, 3] float32, info), info a
    record of _capi.ESSGRAPH_RESULT_DTYPE (iters, nactive, nfailed, nrounds, nlblocks, chi2, lambda).  On a host-only extractor
    the library's host path runs; on the device a problem whose L has more than _capi.ESSGRAPH_MAX_LBLOCKS blocks raises
    OrbxError with status CAPACITY."""
    arr, hold, outs = _essgraph_marshal(problems)
    results = np.zeros(len(problems), _capi.ESSGRAPH_RESULT_DTYPE)
    check(_capi.lib().orbx_optimize_essential_graph_batch(extractor.handle, len(problems), C.cast(arr, C.c_void_p),
                                                          ptr(results) if len(problems) else None))
    return [(S, T, w, results[k]) for k, (S, T, w) in enumerate(outs)]
