"""Microseconds per problem of the batched Optimizer::OptimizeSim3 on the device against the library's own host path.

    python tools/sim3opt_rate.py [--out profiles/sim3opt_batch.md] [--quick]

Device: orbx_optimize_sim3_batch, one call of P = 1, 16, 64, 256 problems with n = 30, 100, 300 correspondences each; the time
is a host clock around the C call, which ends in the wait for the handle's stream, so it contains the packing, the one upload,
the kernel, the one download and the scatter.  Host, in the same run on the same box, alternating with the device: the same
call on a host-only handle (the library's host path: the same scalar code compiled by the host compiler, the problems one after
the other on one core).  That comparison is neither g2o nor the reference: no g2o + Eigen build is timed here.  Half a pixel of
noise, 15 % planted outliers, the start a few degrees, centimetres and percent off; free scale and fixed scale alternate within
a call.  The problems are marshalled once, outside the timed window.  Median, minimum and maximum of the repetitions are
reported; device and host results are compared bit for bit before anything is timed."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sim3opt_scenes as ss  # noqa: E402
from orb_slam2_detailed_comments_amd import ORBextractor, _capi, optimizer  # noqa: E402

SIZES = (1, 16, 64, 256)
CORR = (30, 100, 300)
NSCENES = 16          # distinct scenes per shape; a call of P problems cycles through them


def median_pair(fa, fb, reps):
    fa(); fb()
    ta, tb = [], []
    for _ in range(reps):
        for f, t in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    stat = lambda t: tuple(1e6 * float(f(t)) for f in (np.min, np.median, np.max))
    return stat(ta), stat(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal)")
    ap.add_argument("--host-only", action="store_true", help="rehearse the host column where there is no device (times nothing)")
    a = ap.parse_args()
    L = _capi.lib()
    host = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    dev = host if a.host_only else ORBextractor(1000, 1.2, 8, 20, 7)
    lines = ["| n | P | device, us / problem: median (min - max) | host path, us / problem: median (min - max) | device call, ms |",
             "|---|---|---|---|---|"]
    for n in (CORR[:1] if a.quick else CORR):
        scenes = [ss.make(2000 + k, n, k & 1, noise=0.5, outlier_frac=0.15) for k in range(NSCENES)]
        for P in (SIZES[:2] if a.quick else SIZES):
            probs = [ss.problem(scenes[k % NSCENES]) for k in range(P)]
            arr_d, hold_d, keep_d = optimizer._sim3opt_marshal(probs)
            arr_h, hold_h, keep_h = optimizer._sim3opt_marshal([ss.problem(scenes[k % NSCENES]) for k in range(P)])
            res_d, res_h = np.zeros(P, _capi.SIM3OPT_RESULT_DTYPE), np.zeros(P, _capi.SIM3OPT_RESULT_DTYPE)

            def f_dev():
                _capi.check(L.orbx_optimize_sim3_batch(dev.handle, P, C.cast(arr_d, C.c_void_p), _capi.ptr(res_d)))

            def f_host():
                _capi.check(L.orbx_optimize_sim3_batch(host.handle, P, C.cast(arr_h, C.c_void_p), _capi.ptr(res_h)))

            f_dev(); f_host()
            assert res_d.tobytes() == res_h.tobytes(), "device and host results differ"
            assert all(np.array_equal(x, y) for x, y in zip(keep_d, keep_h)), "device and host keep rows differ"
            if a.host_only:
                print("rehearsal: n %d P %d inliers %.0f" % (n, P, res_h["ninliers"].mean()), flush=True)
                continue
            reps = {1: 400, 16: 60, 64: 20, 256: 6}[P] if n < 300 else {1: 200, 16: 30, 64: 10, 256: 4}[P]
            td, th = median_pair(f_dev, f_host, reps)
            lines.append("| %d | %d | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.3f |"
                         % (n, P, td[1] / P, td[0] / P, td[2] / P, th[1] / P, th[0] / P, th[2] / P, td[1] / 1e3))
            print(lines[-1], "inliers %.0f of %d" % (res_h["ninliers"].mean(), n), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
