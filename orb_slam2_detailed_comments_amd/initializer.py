"""Initializer for monocular initialisation (include/orbx.h): the H / F RANSAC (orbx_init_ransac_batch_create and its
accessors), ReconstructH / ReconstructF with CheckRT and Triangulate (orbx_init_reconstruct_batch_create), and both in one round
trip (orbx_initialize_batch_create).  ctypes marshalling only; `extractor` is the ORBextractor whose handle (stream, staging
block) the batch call runs on.  On a host-only extractor (device=-2) the library's host path runs."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import INIT_F, INIT_H, INIT_NONE, check, ptr  # noqa: F401
from ._ransac import RansacBatch, mask_bits


def _init_problems(problems):
    """(orbx_init_problem array, the arrays it points into, n per problem)"""
    arr = (_capi.InitProblem * max(len(problems), 1))()
    keep, ns = [], []
    for k, p in enumerate(problems):
        k1 = np.ascontiguousarray(p["keys1"], np.float32).reshape(-1, 2)
        k2 = np.ascontiguousarray(p["keys2"], np.float32).reshape(-1, 2)
        m = np.ascontiguousarray(p["matches"], np.int32).reshape(-1, 2)
        sets = p.get("sets")
        if sets is not None:
            sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
            assert len(sets) == int(p["iterations"])
        keep += [k1, k2, m, sets]
        a = arr[k]
        a.n1, a.n2, a.n = len(k1), len(k2), len(m)
        a.keys1 = k1.ctypes.data if len(k1) else None
        a.keys2 = k2.ctypes.data if len(k2) else None
        a.matches = m.ctypes.data if len(m) else None
        a.sigma = float(p["sigma"])
        a.iterations = int(p["iterations"])
        a.sets = sets.ctypes.data if sets is not None and sets.size else None
        a.models = int(p.get("models", INIT_H | INIT_F))
        ns.append(len(m))
    return arr, keep, ns


class InitializerRansac(RansacBatch):
    """problems: dicts with keys1 [n1, 2], keys2 [n2, 2] (float32, ALL keypoints of each frame), matches [n, 2] (int32: index in
    1, index in 2), sigma, iterations, sets [iterations, 8] (the draws in order; not read where n < 8) and models
    (INIT_H | INIT_F, the default).  problems=None: an empty shell that initialize_batch fills."""
    _destroy = "orbx_init_batch_destroy"

    def __init__(self, extractor, problems):
        super().__init__()
        if problems is None:
            return
        arr, keep, self.n = _init_problems(problems)
        check(self._L.orbx_init_ransac_batch_create(extractor.handle, len(problems), C.cast(arr, C.c_void_p), C.byref(self._b)))

    def result(self, k):
        """dict: SH, SF, H21 and F21 (3x3 float32), inliersH and inliersF (bool [n]), itH and itF (-1: none), RH, model"""
        n = self.n[k]
        s = np.zeros(3, np.float32)
        H, F = np.zeros(9, np.float32), np.zeros(9, np.float32)
        iH, iF = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        it = np.zeros(3, np.int32)
        check(self._L.orbx_init_batch_result(self._b, int(k), s[0:].ctypes.data, s[1:].ctypes.data, ptr(H), ptr(F), ptr(iH), ptr(iF),
                                             it[0:].ctypes.data, it[1:].ctypes.data, s[2:].ctypes.data, it[2:].ctypes.data))
        return dict(SH=s[0], SF=s[1], RH=s[2], H21=H.reshape(3, 3), F21=F.reshape(3, 3), inliersH=iH[:n].astype(bool),
                    inliersF=iF[:n].astype(bool), itH=int(it[0]), itF=int(it[1]), model=int(it[2]))

    def scores(self, k, model):
        nit = C.c_int32(0)
        check(self._L.orbx_init_batch_scores(self._b, int(k), int(model), None, C.byref(nit)))
        s = np.zeros(max(nit.value, 1), np.float32)
        check(self._L.orbx_init_batch_scores(self._b, int(k), int(model), ptr(s), C.byref(nit)))
        return s[:nit.value]

    def hypothesis(self, k, model, it):
        """(M 3x3, Minv 3x3 (zeros for F), score, mask bool [n]) of one iteration of one model"""
        n = self.n[k]
        M, Mi = np.zeros(9, np.float32), np.zeros(9, np.float32)
        sc = np.zeros(1, np.float32)
        w = np.zeros(max((n + 63) // 64, 1), np.uint64)
        check(self._L.orbx_init_batch_hypothesis(self._b, int(k), int(model), int(it), ptr(M), ptr(Mi), ptr(sc), ptr(w)))
        return M.reshape(3, 3), Mi.reshape(3, 3), sc[0], mask_bits(w, n)

    def normalization(self, k):
        T1, T2 = np.zeros(9, np.float32), np.zeros(9, np.float32)
        check(self._L.orbx_init_batch_normalization(self._b, int(k), ptr(T1), ptr(T2)))
        return T1.reshape(3, 3), T2.reshape(3, 3)


class InitializerReconstruct(RansacBatch):
    """ReconstructH / ReconstructF for any matrix and mask.  problems: dicts with keys1 [n1, 2], keys2 [n2, 2], matches [n, 2],
    inliers (bool [n], vbMatchesInliers), model (INIT_H: M is H21; INIT_F: M is F21), M (3x3), K (fx, fy, cx, cy), sigma,
    min_parallax (1.0) and min_triangulated (50).  problems=None: an empty shell that initialize_batch fills."""
    _destroy = "orbx_recon_batch_destroy"

    def __init__(self, extractor, problems):
        super().__init__()
        if problems is None:
            return
        arr = (_capi.ReconProblem * max(len(problems), 1))()
        keep = []
        for k, p in enumerate(problems):
            k1 = np.ascontiguousarray(p["keys1"], np.float32).reshape(-1, 2)
            k2 = np.ascontiguousarray(p["keys2"], np.float32).reshape(-1, 2)
            m = np.ascontiguousarray(p["matches"], np.int32).reshape(-1, 2)
            inl = np.ascontiguousarray(p["inliers"]).astype(np.uint8).reshape(-1)
            assert len(inl) == len(m)
            keep += [k1, k2, m, inl]
            a = arr[k]
            a.n1, a.n2, a.n = len(k1), len(k2), len(m)
            a.keys1 = k1.ctypes.data if len(k1) else None
            a.keys2 = k2.ctypes.data if len(k2) else None
            a.matches = m.ctypes.data if len(m) else None
            a.inliers = inl.ctypes.data if len(m) else None
            a.model = int(p["model"])
            a.M[:] = [float(v) for v in np.asarray(p["M"], np.float32).reshape(9)]
            a.K[:] = [float(v) for v in np.asarray(p["K"], np.float32).reshape(4)]
            a.sigma = float(p["sigma"])
            a.min_parallax = float(p.get("min_parallax", 1.0))
            a.min_triangulated = int(p.get("min_triangulated", 50))
            self.n.append(len(m))
        check(self._L.orbx_init_reconstruct_batch_create(extractor.handle, len(problems), C.cast(arr, C.c_void_p), C.byref(self._b)))

    def result(self, k):
        """dict: ok, R21 (3x3) and t21 (3) (zeros when not ok), chosen (the hypothesis the points belong to, -1: none), status
        (uint8 [n] per MATCH: 0 nothing, 1 not finite, 2 counted, 3 counted and triangulated), points (float32 [n, 3]), N"""
        n = self.n[k]
        R, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
        st, pts = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 3), np.float32)
        i = np.zeros(3, np.int32)
        check(self._L.orbx_recon_batch_result(self._b, int(k), i[0:].ctypes.data, ptr(R), ptr(t), i[1:].ctypes.data, ptr(st), ptr(pts),
                                              i[2:].ctypes.data))
        return dict(ok=bool(i[0]), R21=R.reshape(3, 3), t21=t, chosen=int(i[1]), status=st[:n], points=pts[:n], N=int(i[2]))

    def hypothesis(self, k, i):
        """dict: R (3x3), t, n (the plane normal, zeros for F), nGood, cosine, parallax, valid of pose hypothesis i"""
        R, t, nv = np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        f, c = np.zeros(2, np.float32), np.zeros(2, np.int32)
        check(self._L.orbx_recon_batch_hypothesis(self._b, int(k), int(i), ptr(R), ptr(t), ptr(nv), c[0:].ctypes.data, f[0:].ctypes.data,
                                                  f[1:].ctypes.data, c[1:].ctypes.data))
        return dict(R=R.reshape(3, 3), t=t, n=nv, nGood=int(c[0]), cosine=f[0], parallax=f[1], valid=bool(c[1]))


def scatter_matches(result, matches, n1):
    """vP3D [n1, 3] and vbTriangulated [n1] from a result's per-match status and points, in match order (the last write wins,
    a point that is not finite resets the flag): what CheckRT leaves for the chosen hypothesis"""
    P = np.zeros((n1, 3), np.float32)
    good = np.zeros(n1, bool)
    for (first, _), s, pt in zip(np.asarray(matches).reshape(-1, 2), result["status"], result["points"]):
        if s == 1:
            good[first] = False
        elif s >= 2:
            P[first] = pt
            if s == 3:
                good[first] = True
    return P, good


def initialize_batch(extractor, problems, cameras):
    """Initializer::Initialize from the RANSAC to R21, t21, vP3D and vbTriangulated for every problem in one round trip.
    problems as for InitializerRansac; cameras: one dict per problem with K (fx, fy, cx, cy), min_parallax (1.0) and
    min_triangulated (50).  Returns (InitializerRansac, InitializerReconstruct), both to be closed by the caller."""
    assert len(cameras) == len(problems)
    arr, keep, ns = _init_problems(problems)
    cam = (_capi.InitCamera * max(len(problems), 1))()
    for k, c in enumerate(cameras):
        cam[k].K[:] = [float(v) for v in np.asarray(c["K"], np.float32).reshape(4)]
        cam[k].min_parallax = float(c.get("min_parallax", 1.0))
        cam[k].min_triangulated = int(c.get("min_triangulated", 50))
    rb, rc = InitializerRansac(extractor, None), InitializerReconstruct(extractor, None)
    check(rb._L.orbx_initialize_batch_create(extractor.handle, len(problems), C.cast(arr, C.c_void_p), C.cast(cam, C.c_void_p),
                                             C.byref(rb._b), C.byref(rc._b)))
    rb.n, rc.n = list(ns), list(ns)
    return rb, rc
