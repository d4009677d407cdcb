#!/usr/bin/env python3
"""Same-process A/B of the host-fed mono call (orbx_extract_batch, 640x480 gray, 1000 features, chunks of 64) between two builds
of liborbx.so: both libraries are loaded side by side (each ctypes handle resolves its own symbols), each gets its own
page-locked buffers, and the timed rounds alternate A, B, A, B ... so that drifts of the host or the link hit both alike.

    python tools/host_io_ab.py A.so B.so [--frames 256] [--rounds 20] [--calls 10]
"""
import ctypes as C
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from orb_slam2_detailed_comments_amd import synth, _capi

W, H = 640, 480
arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
N, ROUNDS, CALLS = arg("--frames", 256), arg("--rounds", 20), arg("--calls", 10)


class Side:
    def __init__(self, path, frames):
        L = C.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL)
        L.orbx_create.argtypes = [C.POINTER(_capi.Params), C.POINTER(C.c_void_p)]
        L.orbx_default_params.argtypes = [C.POINTER(_capi.Params)]
        L.orbx_max_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.orbx_host_alloc.restype = C.c_void_p; L.orbx_host_alloc.argtypes = [C.c_size_t]
        L.orbx_extract_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int]
        p = _capi.Params()
        L.orbx_default_params(C.byref(p))
        p.nfeatures, p.device, p.max_batch = 1000, 0, 64
        self.h = C.c_void_p()
        assert L.orbx_create(C.byref(p), C.byref(self.h)) == 0
        self.cap = L.orbx_max_keypoints(self.h, W, H)
        pin = lambda shape, dt: np.frombuffer((C.c_uint8 * (int(np.prod(shape)) * np.dtype(dt).itemsize)).from_address(
            L.orbx_host_alloc(int(np.prod(shape)) * np.dtype(dt).itemsize)), dt).reshape(shape)
        self.img = pin((N, H, W), np.uint8); self.img[...] = frames
        self.kps = pin((N, self.cap), _capi.KP_DTYPE); self.desc = pin((N, self.cap, 32), np.uint8); self.cnt = pin((N,), np.int32)
        self.L, self.path = L, path

    def call(self):
        st = self.L.orbx_extract_batch(self.h, N, self.img.ctypes.data, W, H, W, W * H, self.kps.ctypes.data, self.desc.ctypes.data,
                                       self.cnt.ctypes.data, self.cap)
        assert st == 0, st


def main():
    base = synth.stream(W, H, 64, stream_id=100)
    frames = np.concatenate([base] * (N // 64))
    sides = [Side(p, frames) for p in sys.argv[1:3]]
    for s in sides:
        for _ in range(3):
            s.call()
    a, b = sides
    a.call(); b.call()
    assert a.cnt.tobytes() == b.cnt.tobytes() and a.kps.tobytes() == b.kps.tobytes() and a.desc.tobytes() == b.desc.tobytes()
    times = [[], []]
    for r in range(ROUNDS):
        order = (0, 1) if r % 2 == 0 else (1, 0)
        for i in order:
            t = time.perf_counter()
            for _ in range(CALLS):
                sides[i].call()
            times[i].append((time.perf_counter() - t) / CALLS)
    for i, s in enumerate(sides):
        ts = np.array(times[i])
        print(f"{'AB'[i]} {s.path}: {N / np.median(ts):8.0f} frames/s median  [{N / ts.max():.0f} .. {N / ts.min():.0f}]  "
              f"{np.median(ts) * 1e3:.3f} ms per {N}-frame call ({ROUNDS} rounds of {CALLS} calls, alternating)")
    print(f"B / A = {np.median(times[0]) / np.median(times[1]):.4f} (rate ratio; outputs byte-identical)")


if __name__ == "__main__":
    main()
