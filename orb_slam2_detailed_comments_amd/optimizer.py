"""Optimizer::PoseOptimization(Frame*) for tracked frames (include/orbx.h: orbx_pose_optimization_batch_device,
orbx_pose_optimization).  ctypes marshalling only; `extractor` is the ORBextractor whose handle (stream, staging block) the
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
