"""Sim3Solver RANSAC for the candidates of LoopClosing::ComputeSim3 (include/orbx.h: orbx_sim3_ransac_batch_create and the
cursor calls).  ctypes marshalling only; `extractor` is the ORBextractor whose handle (stream, staging block) the batch call runs
on.  One call evaluates every iteration of every problem on the device; iterate() then replays Sim3Solver::iterate on the host.
On a host-only extractor (device=-2) the library's host path runs."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, ptr
from ._ransac import RansacBatch, mask_bits, round_robin


def ransac_iterations(n, probability=0.99, min_inliers=6, max_iterations=300):
    """SetRansacParameters: mRansacMaxIts for a solver with n correspondences"""
    return int(_capi.lib().orbx_sim3_ransac_iterations(int(n), float(probability), int(min_inliers), int(max_iterations)))


class Sim3Ransac(RansacBatch):
    """problems: dicts with x1c, x2c [n, 3], max_err1, max_err2 [n], camera1, camera2 (fx, fy, cx, cy), fix_scale, min_inliers,
    iterations (mRansacMaxIts after SetRansacParameters) and sets [iterations, 3] (the draws in order; not read where
    n < min_inliers)."""
    _destroy = "orbx_sim3_batch_destroy"

    def __init__(self, extractor, problems):
        super().__init__()
        self.extractor = extractor   # compute_sim3_rounds_batched runs OptimizeSim3 on the same handle
        arr = (_capi.Sim3Problem * max(len(problems), 1))()
        keep = []
        for k, p in enumerate(problems):
            x1 = np.ascontiguousarray(p["x1c"], np.float32).reshape(-1, 3)
            x2 = np.ascontiguousarray(p["x2c"], np.float32).reshape(-1, 3)
            e1 = np.ascontiguousarray(p["max_err1"], np.float32).reshape(-1)
            e2 = np.ascontiguousarray(p["max_err2"], np.float32).reshape(-1)
            n = len(x1)
            assert len(x2) == n and len(e1) == n and len(e2) == n
            sets = p.get("sets")
            if sets is not None:
                sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 3)
                assert len(sets) == int(p["iterations"])
            keep += [x1, x2, e1, e2, sets]
            a = arr[k]
            a.n = n
            a.x1c, a.x2c, a.max_err1, a.max_err2 = (v.ctypes.data if n else None for v in (x1, x2, e1, e2))
            a.camera1[:] = np.asarray(p["camera1"], np.float32).tolist()
            a.camera2[:] = np.asarray(p["camera2"], np.float32).tolist()
            a.fix_scale = int(bool(p["fix_scale"]))
            a.min_inliers = int(p["min_inliers"])
            a.iterations = int(p["iterations"])
            a.sets = sets.ctypes.data if sets is not None and sets.size else None
            self.n.append(n)
        check(self._L.orbx_sim3_ransac_batch_create(extractor.handle, len(problems), C.cast(arr, C.c_void_p), C.byref(self._b)))
        self.iterations = [int(p["iterations"]) for p in problems]

    def iterate(self, k, n_iterations):
        """Sim3Solver::iterate of solver k: (T12 4x4 float32 or None, no_more, inliers bool [n], ninliers)"""
        n = self.n[k]
        inl = np.zeros(max(n, 1), np.uint8)
        T = np.zeros(16, np.float32)
        no_more, nin = C.c_int32(0), C.c_int32(0)
        r = self._L.orbx_sim3_batch_iterate(self._b, int(k), int(n_iterations), C.byref(no_more), ptr(inl), C.byref(nin), ptr(T))
        if r < 0:
            check(_capi.BAD_ARGUMENT)
        return (T.reshape(4, 4) if r == 1 else None), bool(no_more.value), inl[:n].astype(bool), int(nin.value)

    def best(self, k):
        """GetEstimatedRotation / Translation / Scale of solver k"""
        R, t, s = np.zeros(9, np.float32), np.zeros(3, np.float32), C.c_float(0)
        check(self._L.orbx_sim3_batch_best(self._b, int(k), ptr(R), ptr(t), C.byref(s)))
        return R.reshape(3, 3), t, np.float32(s.value)

    def counts(self, k):
        c = np.zeros(max(self.iterations[k], 1), np.int32)
        nit = C.c_int32(0)
        check(self._L.orbx_sim3_batch_counts(self._b, int(k), ptr(c), C.byref(nit)))
        return c[:nit.value]

    def hypothesis(self, k, iteration):
        """(48 floats: T12 | T21 | R | t | s | 0 0 0, mask bool [n]) of one stored iteration"""
        n = self.n[k]
        h = np.zeros(48, np.float32)
        w = np.zeros(max((n + 63) // 64, 1), np.uint64)
        check(self._L.orbx_sim3_batch_hypothesis(self._b, int(k), int(iteration), ptr(h), ptr(w)))
        return h, mask_bits(w, n)


def compute_sim3_round_robin(ransac, accept, n_iterations=5):
    """The candidate loop of LoopClosing::ComputeSim3 (src/LoopClosing.cc:487-577) over the solvers of `ransac` (anything with
    __len__ and iterate(k, n)): every live solver gets iterate(n_iterations) in turn; a solver that reports no_more is
    discarded; accept(k, T12, inliers, ninliers) -- OptimizeSim3 and the >= 20 test in the reference -- ends the loop when it
    returns true.  Returns the accepted solver's index or -1, and the list of (k, returned, no_more, ninliers) calls made."""
    return round_robin(ransac, accept, n_iterations)


def compute_sim3_rounds_batched(ransac, prepare, n_iterations=5, min_inliers=20, extractor=None):
    """The candidate loop of LoopClosing::ComputeSim3 with OptimizeSim3 batched per round: every live solver gets
    iterate(n_iterations); prepare(k, T12, inliers) -- the caller's SearchBySim3 -- gives an optimize_sim3_batch problem (or None)
    for each solver that returned a Sim3; ONE optimize_sim3_batch call serves the round, and the lowest k with
    ninliers >= min_inliers is accepted.  Returns (k or -1, calls, result record or None, keep or None); calls as
    compute_sim3_round_robin lists them.  The one difference from compute_sim3_round_robin: solvers after the accepted one have
    been iterated in the final round (the reference destroys them at that point anyway).  extractor: the ORBextractor whose handle
    the batch runs on (default: ransac.extractor)."""
    from .optimizer import optimize_sim3_batch
    ex = extractor if extractor is not None else ransac.extractor
    K = len(ransac)
    discarded = [False] * K
    live = K
    calls = []
    while live > 0:
        ks, problems = [], []
        for k in range(K):
            if discarded[k]:
                continue
            T, no_more, inl, nin = ransac.iterate(k, n_iterations)
            calls.append((k, T is not None, no_more, nin))
            if no_more:
                discarded[k] = True
                live -= 1
            if T is not None:
                p = prepare(k, T, inl)
                if p is not None:
                    ks.append(k)
                    problems.append(p)
        if problems:
            results, keeps = optimize_sim3_batch(ex, problems)
            for j, k in enumerate(ks):
                if results[j]["ninliers"] >= min_inliers:
                    return k, calls, results[j].copy(), keeps[j]
    return -1, calls, None, None


def compute_sim3_rounds_device(ransac, matcher, keyframes, search, optimize, camera4, bounds4, n_iterations=5, min_inliers=20,
                               extractor=None):
    """compute_sim3_rounds_batched with SearchBySim3 batched as well: every stage of a round is one device round trip.  Every
    live solver gets iterate(n_iterations); search(k, T12, inliers) gives the ORBmatcher.SearchBySim3Batch problem of each solver
    that returned a Sim3 (kf1, kf2 as indices into `keyframes`, s12, R12, t12, th, matched1, matched2 -- or None); ONE
    matcher.SearchBySim3Batch call serves the round; optimize(k, T12, inliers, matches12, nfound) turns a solver's matches into its
    optimize_sim3_batch problem (or None); ONE optimize_sim3_batch call follows, and the lowest k with ninliers >= min_inliers is
    accepted.  Returns what compute_sim3_rounds_batched returns when its prepare runs the single SearchBySim3 between the same
    two callbacks."""
    from .optimizer import optimize_sim3_batch
    ex = extractor if extractor is not None else ransac.extractor
    K = len(ransac)
    discarded = [False] * K
    live = K
    calls = []
    while live > 0:
        found = []
        for k in range(K):
            if discarded[k]:
                continue
            T, no_more, inl, nin = ransac.iterate(k, n_iterations)
            calls.append((k, T is not None, no_more, nin))
            if no_more:
                discarded[k] = True
                live -= 1
            if T is not None:
                sp = search(k, T, inl)
                if sp is not None:
                    found.append((k, T, inl, sp))
        if not found:
            continue
        counts, matches = matcher.SearchBySim3Batch(keyframes, [f[3] for f in found], camera4, bounds4)
        ks, problems = [], []
        for j, (k, T, inl, _) in enumerate(found):
            p = optimize(k, T, inl, matches[j], counts[j])
            if p is not None:
                ks.append(k)
                problems.append(p)
        if problems:
            results, keeps = optimize_sim3_batch(ex, problems)
            for j, k in enumerate(ks):
                if results[j]["ninliers"] >= min_inliers:
                    return k, calls, results[j].copy(), keeps[j]
    return -1, calls, None, None
