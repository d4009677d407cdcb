"""Initializer H / F RANSAC for monocular initialisation (include/orbx.h: orbx_init_ransac_batch_create and its accessors).
ctypes marshalling only; `extractor` is the ORBextractor whose handle (stream, staging block) the batch call runs on.  One call
evaluates every iteration of both models of every problem on the device and picks the best iteration of each model.  On a
host-only extractor (device=-2) the library's host path runs."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import INIT_F, INIT_H, INIT_NONE, check, ptr  # noqa: F401
from ._ransac import RansacBatch, mask_bits


class InitializerRansac(RansacBatch):
    """problems: dicts with keys1 [n1, 2], keys2 [n2, 2] (float32, ALL keypoints of each frame), matches [n, 2] (int32: index in
    1, index in 2), sigma, iterations, sets [iterations, 8] (the draws in order; not read where n < 8) and models
    (INIT_H | INIT_F, the default)."""
    _destroy = "orbx_init_batch_destroy"

    def __init__(self, extractor, problems):
        super().__init__()
        arr = (_capi.InitProblem * max(len(problems), 1))()
        keep = []
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
            self.n.append(len(m))
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
