"""PnPsolver (EPnP RANSAC) for the candidates of Tracking::Relocalization (include/orbx.h: orbx_pnp_ransac_batch_create and the
cursor calls).  ctypes marshalling only; `extractor` is the ORBextractor whose handle (stream, staging block) the batch call runs
on.  One call evaluates every iteration of every problem on the device; iterate() then replays PnPsolver::iterate on the host,
Refine included.  On a host-only extractor (device=-2) the library's host path runs."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, ptr
from ._ransac import RansacBatch, mask_bits, round_robin


def pnp_ransac_parameters(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """SetRansacParameters: (mRansacMinInliers, mRansacMaxIts) for a solver with n correspondences"""
    mi, it = C.c_int32(0), C.c_int32(0)
    _capi.lib().orbx_pnp_ransac_parameters(int(n), float(probability), int(min_inliers), int(max_iterations), int(min_set),
                                           float(epsilon), C.byref(mi), C.byref(it))
    return int(mi.value), int(it.value)


class PnPRansac(RansacBatch):
    """problems: dicts with p3dw [n, 3], p2d [n, 2], max_err [n] (float32), camera (fu, fv, uc, vc as doubles), min_inliers and
    iterations (both after SetRansacParameters) and sets [iterations, 4] (the draws in order; not read where n < min_inliers)."""
    _destroy = "orbx_pnp_batch_destroy"

    def __init__(self, extractor, problems):
        super().__init__()
        arr = (_capi.PnpProblem * max(len(problems), 1))()
        keep = []
        for k, p in enumerate(problems):
            p3 = np.ascontiguousarray(p["p3dw"], np.float32).reshape(-1, 3)
            p2 = np.ascontiguousarray(p["p2d"], np.float32).reshape(-1, 2)
            me = np.ascontiguousarray(p["max_err"], np.float32).reshape(-1)
            n = len(p3)
            assert len(p2) == n and len(me) == n
            sets = p.get("sets")
            if sets is not None:
                sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 4)
                assert len(sets) == int(p["iterations"])
            keep += [p3, p2, me, sets]
            a = arr[k]
            a.n = n
            a.p3dw, a.p2d, a.max_err = (v.ctypes.data if n else None for v in (p3, p2, me))
            a.camera[:] = [float(c) for c in p["camera"]]
            a.min_inliers = int(p["min_inliers"])
            a.iterations = int(p["iterations"])
            a.sets = sets.ctypes.data if sets is not None and sets.size else None
            self.n.append(n)
        check(self._L.orbx_pnp_ransac_batch_create(extractor.handle, len(problems), C.cast(arr, C.c_void_p), C.byref(self._b)))

    def iterate(self, k, n_iterations, draw=None):
        """PnPsolver::iterate of solver k: (Tcw 4x4 float32 or None, no_more, inliers bool [n], ninliers).  When the replay needs
        iterations past those stored, draw(k, count) must return count further sets [count, 4]; they are appended and the call is
        repeated.  Without draw such a call raises."""
        n = self.n[k]
        inl = np.zeros(max(n, 1), np.uint8)
        T = np.zeros(16, np.float32)
        no_more, nin = C.c_int32(0), C.c_int32(0)
        while True:
            r = self._L.orbx_pnp_batch_iterate(self._b, int(k), int(n_iterations), C.byref(no_more), ptr(inl), C.byref(nin), ptr(T))
            if r != -2:
                break
            if draw is None:
                raise RuntimeError("PnPRansac.iterate: the replay needs iterations past those stored and no draw was given")
            self.append(k, draw(k, max(int(n_iterations), 1)))
        if r < 0:
            check(_capi.BAD_ARGUMENT)
        return (T.reshape(4, 4) if r == 1 else None), bool(no_more.value), inl[:n].astype(bool), int(nin.value)

    def iterate_raw(self, k, n_iterations):
        """the cursor's own return value (1, 0, -1, -2) with the same outputs"""
        n = self.n[k]
        inl = np.zeros(max(n, 1), np.uint8)
        T = np.zeros(16, np.float32)
        no_more, nin = C.c_int32(0), C.c_int32(0)
        r = self._L.orbx_pnp_batch_iterate(self._b, int(k), int(n_iterations), C.byref(no_more), ptr(inl), C.byref(nin), ptr(T))
        return int(r), T.reshape(4, 4), bool(no_more.value), inl[:n].astype(bool), int(nin.value)

    def append(self, k, sets):
        sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 4)
        check(self._L.orbx_pnp_batch_append(self._b, int(k), len(sets), ptr(sets) if len(sets) else None))

    def best(self, k):
        """(mBestTcw 4x4, mnBestInliers, the iteration behind them)"""
        T = np.zeros(16, np.float32)
        nin, it = C.c_int32(0), C.c_int32(0)
        check(self._L.orbx_pnp_batch_best(self._b, int(k), ptr(T), C.byref(nin), C.byref(it)))
        return T.reshape(4, 4), int(nin.value), int(it.value)

    def counts(self, k):
        nit = C.c_int32(0)
        check(self._L.orbx_pnp_batch_counts(self._b, int(k), None, C.byref(nit)))
        c = np.zeros(max(nit.value, 1), np.int32)
        check(self._L.orbx_pnp_batch_counts(self._b, int(k), ptr(c), C.byref(nit)))
        return c[:nit.value]

    def hypothesis(self, k, iteration):
        """(R | t as 12 doubles, Tcw 16 floats, N, mask bool [n]) of one stored iteration"""
        n = self.n[k]
        rt = np.zeros(12, np.float64)
        T = np.zeros(16, np.float32)
        N = C.c_int32(0)
        w = np.zeros(max((n + 63) // 64, 1), np.uint64)
        check(self._L.orbx_pnp_batch_hypothesis(self._b, int(k), int(iteration), ptr(rt), ptr(T), C.byref(N), ptr(w)))
        return rt, T, int(N.value), mask_bits(w, n)


def relocalization_round_robin(ransac, accept, n_iterations=5, draw=None):
    """The candidate loop of Tracking::Relocalization (src/Tracking.cc:2336-2366 and what follows per candidate) over the solvers
    of `ransac` (anything with __len__ and iterate(k, n, draw)): every live solver gets iterate(n_iterations) in turn; a solver
    that reports no_more is discarded; accept(k, Tcw, inliers, ninliers) -- PoseOptimization, the guided searches and the >= 50
    test in the reference -- ends the loop when it returns true.  Returns the accepted solver's index or -1, and the list of
    (k, returned, no_more, ninliers) calls made."""
    return round_robin(ransac, accept, n_iterations, draw)
