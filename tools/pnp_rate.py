"""Microseconds per candidate of the batched PnPsolver RANSAC on the device against the library's own host path.

    python tools/pnp_rate.py [--out <table.md>] [--quick]

Device: orbx_pnp_ransac_batch_create, one call of P = 1, 16, 64 problems (the candidate keyframes of one
Tracking::Relocalization), every problem with N = 30, 100 or 300 correspondences and 35 iterations (what SetRansacParameters
(0.99, 10, 300, 4, 0.5, 5.991) gives from N = 20 upwards); the time is a host clock around the C call, which returns after its
one download, so it contains the packing, the upload, both kernels, the download and the scatter of the results into the batch.
The ctypes problem array is built before the clock starts.  Host, in the same run on the same box, alternating with the device:
the same call on a host-only handle (the library's host path: the same scalar code compiled by the host compiler, the problems
one after the other on one core).  That host path is neither the reference nor OpenCV.  Median, minimum and maximum of the
repetitions (300 / 100 / 30 for P = 1 / 16 / 64) are reported; device and host results are compared bit for bit before anything
is timed.  No threshold is set: the table says what was measured, a single candidate losing to the host included."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pnp_scenes as ps  # noqa: E402
from orb_slam2_detailed_comments_amd import ORBextractor, _capi  # noqa: E402

SIZES = (1, 16, 64)
NS = (30, 100, 300)
ITERATIONS = 35
REPS = {1: 300, 16: 100, 64: 30}


def marshal(problems):
    arr = (_capi.PnpProblem * len(problems))()
    keep = []
    for a, p in zip(arr, problems):
        bufs = [np.ascontiguousarray(p[k], np.float32) for k in ("p3dw", "p2d", "max_err")]
        sets = np.ascontiguousarray(p["sets"], np.int32)
        keep += bufs + [sets]
        a.n = len(bufs[0])
        a.p3dw, a.p2d, a.max_err = (b.ctypes.data for b in bufs)
        a.camera[:] = list(p["camera"])
        a.min_inliers, a.iterations, a.sets = p["min_inliers"], p["iterations"], sets.ctypes.data
    return arr, keep


def create(L, handle, arr, n):
    b = C.c_void_p()
    _capi.check(L.orbx_pnp_ransac_batch_create(handle, n, C.cast(arr, C.c_void_p), C.byref(b)))
    return b


def results(L, b, problems):
    out = []
    for k, p in enumerate(problems):
        c = np.zeros(p["iterations"], np.int32)
        _capi.check(L.orbx_pnp_batch_counts(b, k, _capi.ptr(c), None))
        rt = np.zeros((p["iterations"], 12), np.float64)
        T = np.zeros((p["iterations"], 16), np.float32)
        N = np.zeros(p["iterations"], np.int32)
        w = np.zeros((p["iterations"], (len(p["p3dw"]) + 63) // 64), np.uint64)
        for i in range(p["iterations"]):
            n1 = C.c_int32(0)
            _capi.check(L.orbx_pnp_batch_hypothesis(b, k, i, _capi.ptr(rt[i]), _capi.ptr(T[i]), C.byref(n1), _capi.ptr(w[i])))
            N[i] = n1.value
        out.append((c, rt.view(np.uint64), T.view(np.uint32), N, w))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a tenth of the repetitions")
    args = ap.parse_args()
    L = _capi.lib()
    dev = ORBextractor(1000, 1.2, 8, 20, 7)
    host = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    rows = []
    for n in NS:
        for P in SIZES:
            problems = [ps.make(5000 + 100 * n + k, n, 0.3, iterations=ITERATIONS, noise=0.3) for k in range(P)]
            arr, keep = marshal(problems)
            bd, bh = create(L, dev.handle, arr, P), create(L, host.handle, arr, P)
            for rd, rh in zip(results(L, bd, problems), results(L, bh, problems)):
                assert all(np.array_equal(x, y) for x, y in zip(rd, rh)), "device and host path differ"
            L.orbx_pnp_batch_destroy(bd); L.orbx_pnp_batch_destroy(bh)
            reps = max(3, REPS[P] // (10 if args.quick else 1))
            for _ in range(3):                                 # warm-up of this shape on both paths
                L.orbx_pnp_batch_destroy(create(L, dev.handle, arr, P)); L.orbx_pnp_batch_destroy(create(L, host.handle, arr, P))
            td, th = [], []
            for _ in range(reps):
                for handle, t in ((dev.handle, td), (host.handle, th)):
                    t0 = time.perf_counter()
                    b = create(L, handle, arr, P)
                    t.append(time.perf_counter() - t0)
                    L.orbx_pnp_batch_destroy(b)
            td, th = np.array(td) * 1e6 / P, np.array(th) * 1e6 / P
            rows.append((n, P, reps, td, th))
            print(f"N {n:4d}  P {P:3d}  reps {reps:4d}  device {np.median(td):9.1f} ({td.min():.1f} - {td.max():.1f}) us/candidate   "
                  f"host {np.median(th):9.1f} ({th.min():.1f} - {th.max():.1f})   x{np.median(th) / np.median(td):.2f}   "
                  f"device call {np.median(td) * P / 1e3:.3f} ms", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("| N | P | repetitions | device, us / candidate: median (min - max) | host path, us / candidate: median (min - max) | host / device | device call, ms |\n")
            f.write("|---|---|---|---|---|---|---|\n")
            for n, P, reps, td, th in rows:
                f.write(f"| {n} | {P} | {reps} | {np.median(td):.1f} ({td.min():.1f} - {td.max():.1f}) | {np.median(th):.1f} ({th.min():.1f} - {th.max():.1f}) | "
                        f"{np.median(th) / np.median(td):.2f} | {np.median(td) * P / 1e3:.3f} |\n")
    dev.close(); host.close()


if __name__ == "__main__":
    main()
