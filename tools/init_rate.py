"""Microseconds per initialisation attempt of the batched Initializer H / F RANSAC on the device against the library's own host
path.

    python tools/init_rate.py [--out <table.md>] [--quick]

Device: orbx_init_ransac_batch_create, one call of P = 1, 16, 64, 256 problems (the outstanding initialisation attempts of a
tracker that feeds many streams), every problem with n = 100, 300 or 1000 matches among 1.5 n keypoints per frame, 200 iterations
and both models (mMaxIterations = 200 is what Tracking hands the Initializer); the time is a host clock around the C call, which
returns after its one download, so it contains validation, Normalize, the packing, the upload, both kernels, the download and the
scatter of the results into the batch.  The ctypes problem array is built before the clock starts.  Host, in the same run on the
same box, alternating with the device: the same call on a host-only handle (the library's host path: the same scalar code
compiled by the host compiler, the problems one after the other on one core).  That host path is neither the reference nor
OpenCV.  Median, minimum and maximum of the repetitions (100 / 30 / 10 / 5 for P = 1 / 16 / 64 / 256) are reported; device and
host results are compared bit for bit before anything is timed.  No threshold is set: the table says what was measured, a single
attempt losing to the host included."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import init_scenes as sc  # noqa: E402
from orb_slam2_detailed_comments_amd import ORBextractor, _capi  # noqa: E402

SIZES = (1, 16, 64, 256)
NS = (100, 300, 1000)
ITERATIONS = 200
REPS = {1: 100, 16: 30, 64: 10, 256: 5}


def marshal(problems):
    arr = (_capi.InitProblem * len(problems))()
    keep = []
    for a, p in zip(arr, problems):
        k1, k2 = np.ascontiguousarray(p["keys1"], np.float32), np.ascontiguousarray(p["keys2"], np.float32)
        m, sets = np.ascontiguousarray(p["matches"], np.int32), np.ascontiguousarray(p["sets"], np.int32)
        keep += [k1, k2, m, sets]
        a.n1, a.n2, a.n = len(k1), len(k2), len(m)
        a.keys1, a.keys2, a.matches, a.sets = k1.ctypes.data, k2.ctypes.data, m.ctypes.data, sets.ctypes.data
        a.sigma, a.iterations, a.models = float(p["sigma"]), int(p["iterations"]), int(p["models"])
    return arr, keep


def create(L, handle, arr, n):
    b = C.c_void_p()
    _capi.check(L.orbx_init_ransac_batch_create(handle, n, C.cast(arr, C.c_void_p), C.byref(b)))
    return b


def results(L, b, problems):
    out = []
    for k, p in enumerate(problems):
        it, nw = p["iterations"], (len(p["matches"]) + 63) // 64
        M, Mi = np.zeros((2, it, 9), np.float32), np.zeros((2, it, 9), np.float32)
        s, w = np.zeros((2, it), np.float32), np.zeros((2, it, nw), np.uint64)
        for mi, model in enumerate((1, 2)):
            for i in range(it):
                _capi.check(L.orbx_init_batch_hypothesis(b, k, model, i, _capi.ptr(M[mi, i]), _capi.ptr(Mi[mi, i]),
                                                         s[mi, i:].ctypes.data, _capi.ptr(w[mi, i])))
        out.append((M.view(np.uint32), Mi.view(np.uint32), s.view(np.uint32), w))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a fifth of the repetitions")
    args = ap.parse_args()
    L = _capi.lib()
    dev = ORBextractor(1000, 1.2, 8, 20, 7)
    host = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    rows = []
    for n in NS:
        base = [sc.make(7000 + n + k, n, ("general", "plane", "rotation", "general")[k % 4], iterations=ITERATIONS, extra1=n // 2,
                        extra2=n // 2) for k in range(8)]
        for P in SIZES:
            problems = [base[k % 8] for k in range(P)]          # the same eight scenes over and over: the work per attempt is what counts
            arr, keep = marshal(problems)
            if P <= 16:
                bd, bh = create(L, dev.handle, arr, P), create(L, host.handle, arr, P)
                for rd, rh in zip(results(L, bd, problems), results(L, bh, problems)):
                    assert all(np.array_equal(x, y) for x, y in zip(rd, rh)), "device and host path differ"
                L.orbx_init_batch_destroy(bd); L.orbx_init_batch_destroy(bh)
            reps = max(3, REPS[P] // (5 if args.quick else 1))
            for _ in range(2):                                 # warm-up of this shape on both paths
                L.orbx_init_batch_destroy(create(L, dev.handle, arr, P)); L.orbx_init_batch_destroy(create(L, host.handle, arr, P))
            td, th = [], []
            for _ in range(reps):
                for handle, t in ((dev.handle, td), (host.handle, th)):
                    t0 = time.perf_counter()
                    b = create(L, handle, arr, P)
                    t.append(time.perf_counter() - t0)
                    L.orbx_init_batch_destroy(b)
            td, th = np.array(td) * 1e6 / P, np.array(th) * 1e6 / P
            rows.append((n, P, reps, td, th))
            print(f"n {n:4d}  P {P:3d}  reps {reps:4d}  device {np.median(td):9.1f} ({td.min():.1f} - {td.max():.1f}) us/attempt   "
                  f"host {np.median(th):9.1f} ({th.min():.1f} - {th.max():.1f})   x{np.median(th) / np.median(td):.2f}   "
                  f"device call {np.median(td) * P / 1e3:.3f} ms", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("| n | P | repetitions | device, us / attempt: median (min - max) | host path, us / attempt: median (min - max) | host / device | device call, ms |\n")
            f.write("|---|---|---|---|---|---|---|\n")
            for n, P, reps, td, th in rows:
                f.write(f"| {n} | {P} | {reps} | {np.median(td):.1f} ({td.min():.1f} - {td.max():.1f}) | {np.median(th):.1f} ({th.min():.1f} - {th.max():.1f}) | "
                        f"{np.median(th) / np.median(td):.2f} | {np.median(td) * P / 1e3:.3f} |\n")
    dev.close(); host.close()


if __name__ == "__main__":
    main()
