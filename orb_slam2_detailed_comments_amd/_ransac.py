"""What the batched RANSAC wrappers (sim3.py, pnp.py, initializer.py) share: the ownership of the C batch object, the unpacking
of mask words and the round-robin loop over the solvers of a batch."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi


class RansacBatch:
    """Owns the batch pointer `_b` a subclass's orbx_*_ransac_batch_create fills; `_destroy` names the C call that frees it.
    `n` is the number of correspondences of each problem."""
    _destroy = None

    def __init__(self):
        self._L = _capi.lib()
        self._b = C.c_void_p()
        self.n = []

    def __len__(self):
        return len(self.n)

    def close(self):
        if self._b:
            getattr(self._L, self._destroy)(self._b)
            self._b = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mask_bits(words, n):
    """bool [n] of the 64-bit mask words: bit i of word w is correspondence 64 w + i"""
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def round_robin(ransac, accept, n_iterations, *iterate_args):
    """Every live solver of `ransac` (anything with __len__ and iterate(k, n, *iterate_args)) gets iterate(n_iterations) in turn;
    a solver that reports no_more is discarded; accept(k, T, inliers, ninliers) ends the loop when it returns true.  Returns the
    accepted solver's index or -1, and the list of (k, returned, no_more, ninliers) calls made."""
    K = len(ransac)
    discarded = [False] * K
    live = K
    calls = []
    while live > 0:
        for k in range(K):
            if discarded[k]:
                continue
            T, no_more, inl, nin = ransac.iterate(k, n_iterations, *iterate_args)
            calls.append((k, T is not None, no_more, nin))
            if no_more:
                discarded[k] = True
                live -= 1
            if T is not None and accept(k, T, inl, nin):
                return k, calls
    return -1, calls
