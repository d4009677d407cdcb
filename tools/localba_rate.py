"""Milliseconds per problem of the batched Optimizer::LocalBundleAdjustment on the device against the library's own host path.

    python tools/localba_rate.py [--out profiles/localba_batch.md] [--quick] [--host-only]

Device: orbx_local_bundle_adjustment_batch, one call of B = 1, 4, 16, 64 problems of two sizes (about 8 local + 8 fixed
keyframes, 600 points, 3 500 edges; about 25 local + 20 fixed keyframes, 2 000 points, 14 000 edges); the time is a host clock
around the C call, which ends in the wait for the handle's stream, so it contains the validation, the derived index lists, the
packing, the one upload, the kernel, the one download and the scatter.  Host, in the same run on the same box, alternating with
the device: the same call on a host-only handle (the library's host path: the same scalar code compiled by the host compiler,
the problems one after the other on one core).  That comparison is neither g2o nor the reference: no g2o + Eigen build is timed
here.  0.7 level sigmas of noise, 10 % planted outliers, the start centimetres and a fraction of a degree off.  The problems
are marshalled once, outside the timed window.  Median, minimum and maximum of the repetitions are reported (20 device calls
per row; the host path's time per problem does not depend on B, so its rows at B = 16 and 64 take 5 and 3 calls); device and
host results are compared bit for bit before anything is timed."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import localba_scenes as sc  # noqa: E402
from orb_slam2_detailed_comments_amd import ORBextractor, _capi, optimizer  # noqa: E402

BATCHES = (1, 4, 16, 64)
SHAPES = (("8 + 8 keyframes, 600 points", dict(nlocal=8, nfixed=8, npoints=600, min_obs=2, max_obs=10)),
          ("25 + 20 keyframes, 2000 points", dict(nlocal=25, nfixed=20, npoints=2000, min_obs=2, max_obs=12)))
NSCENES = 4           # distinct scenes per shape; a call of B problems cycles through them
HOST_REPS = {1: 20, 4: 20, 16: 5, 64: 3}


def timed(f, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return tuple(1e3 * float(g(t)) for g in (np.min, np.median, np.max))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the small shape at B = 1, 4 only (a rehearsal)")
    ap.add_argument("--host-only", action="store_true", help="rehearse the host column where there is no device (times nothing)")
    a = ap.parse_args()
    L = _capi.lib()
    host = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    dev = host if a.host_only else ORBextractor(1000, 1.2, 8, 20, 7)
    lines = ["| problem | edges | B | device, ms / problem: median (min - max) | host path, ms / problem: median (min - max) | device call, ms |",
             "|---|---|---|---|---|---|"]
    for name, kw in (SHAPES[:1] if a.quick else SHAPES):
        scenes = [sc.make(3000 + k, noise=0.7, outlier_frac=0.1, **kw) for k in range(NSCENES)]
        edges = int(np.mean([len(s["obs_kf"]) for s in scenes]))
        for B in (BATCHES[:2] if a.quick else BATCHES):
            arr_d, hold_d, out_d = optimizer._localba_marshal([scenes[k % NSCENES] for k in range(B)])
            arr_h, hold_h, out_h = optimizer._localba_marshal([scenes[k % NSCENES] for k in range(B)])
            res_d, res_h = np.zeros(B, _capi.LOCALBA_RESULT_DTYPE), np.zeros(B, _capi.LOCALBA_RESULT_DTYPE)

            def f_dev():
                _capi.check(L.orbx_local_bundle_adjustment_batch(dev.handle, B, C.cast(arr_d, C.c_void_p), _capi.ptr(res_d)))

            def f_host():
                _capi.check(L.orbx_local_bundle_adjustment_batch(host.handle, B, C.cast(arr_h, C.c_void_p), _capi.ptr(res_h)))

            f_dev(); f_host()                                   # warm-up, and the check
            assert res_d.tobytes() == res_h.tobytes(), "device and host results differ"
            for (Td, wd, ed), (Th, wh, eh) in zip(out_d, out_h):
                assert Td.tobytes() == Th.tobytes() and wd.tobytes() == wh.tobytes() and ed.tobytes() == eh.tobytes(), "device and host differ"
            f_dev()
            td, th = timed(f_dev, 20), timed(f_host, HOST_REPS[B])
            lines.append("| %s | %d | %d | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.2f |" % (
                name, edges, B, td[1] / B, td[0] / B, td[2] / B, th[1] / B, th[0] / B, th[2] / B, td[1]))
            print(lines[-1], flush=True)
            it = [int(r["iters"][0]) + int(r["iters"][1]) for r in res_d]
        lines.append("| | | | iterations per problem (both rounds): %s | | |" % sorted(set(it)))
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
