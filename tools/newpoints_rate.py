"""Microseconds per problem of the batched per-match geometry of LocalMapping::CreateNewMapPoints on the device against the
library's own host path.

    python tools/newpoints_rate.py [--out FILE] [--quick] [--host-only]

Device: orbx_create_new_map_points_batch, one call of P = 1, 16, 256 problems with n = 30, 100, 300 matches each; the time is a
host clock around the C call, which ends in the wait for the handle's stream, so it contains the validation, the gather of the
operands into planes, the one upload, the kernel, the one download and the scatter.  Host, in the same run on the same box,
alternating with the device: the same call on a host-only handle (the library's host path: the same scalar code compiled by the
host compiler, the matches one after the other on one core).  That comparison is neither the reference nor OpenCV: no OpenCV
build is timed here.  The scenes are tests/newpoints_scenes.py's general scene (a wide baseline, half a pixel of noise, every
stereo combination, one outlier in eleven), 16 seeds per shape; a call of more problems cycles through them.  The problems are
marshalled once, outside the timed window.  Median, minimum and maximum of the repetitions are reported; device and host results
are compared bit for bit before anything is timed."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import newpoints_scenes as sc  # noqa: E402
from orb_slam2_detailed_comments_amd import ORBextractor, _capi, localmapping  # noqa: E402

SIZES = (1, 16, 256)
MATCHES = (30, 100, 300)
NSCENES = 16          # distinct scenes per shape; a call of P problems cycles through them
REPS = {1: 400, 16: 100, 256: 12}


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
    for n in (MATCHES[:1] if a.quick else MATCHES):
        scenes = [sc.general(n, seed=3000 + k) for k in range(NSCENES)]
        for P in (SIZES[:2] if a.quick else SIZES):
            probs = [scenes[k % NSCENES] for k in range(P)]
            arr, keep, counts = localmapping._newpoints_marshal(probs)
            total = sum(counts)
            st_d, st_h = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
            pt_d, pt_h = np.zeros((total, 3), np.float32), np.zeros((total, 3), np.float32)

            def f_dev():
                _capi.check(L.orbx_create_new_map_points_batch(dev.handle, P, C.cast(arr, C.c_void_p), _capi.ptr(st_d), _capi.ptr(pt_d)))

            def f_host():
                _capi.check(L.orbx_create_new_map_points_batch(host.handle, P, C.cast(arr, C.c_void_p), _capi.ptr(st_h), _capi.ptr(pt_h)))

            f_dev(); f_host()
            assert st_d.tobytes() == st_h.tobytes() and pt_d.tobytes() == pt_h.tobytes(), "device and host results differ"
            accepted = float(np.isin(st_h, localmapping.ACCEPTED).mean())
            if a.host_only:
                print("rehearsal: n %d P %d accepted %.2f" % (n, P, accepted), flush=True)
                continue
            td, th = median_pair(f_dev, f_host, REPS[P])
            lines.append("| %d | %d | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.3f |"
                         % (n, P, td[1] / P, td[0] / P, td[2] / P, th[1] / P, th[0] / P, th[2] / P, td[1] / 1e3))
            print(lines[-1], "accepted %.2f" % accepted, flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
