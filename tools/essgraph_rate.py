"""Milliseconds per problem of the batched Optimizer::OptimizeEssentialGraph on the device against the library's own host path.

    python tools/essgraph_rate.py [--out profiles/essgraph_batch.md] [--quick] [--host-only]

Device: orbx_optimize_essential_graph_batch, one call of B = 1, 4, 16, 64 problems of three sizes: chains of 100, 400 and 1500
keyframes with covisibility edges to the three keyframes before the parent (tests/essgraph_scenes.chain_covis), keyframe 0
fixed, one map point per keyframe and ten; the time is a host clock around the C call, which ends in the wait for the handle's
stream, so it contains the validation, the elimination order and the symbolic factorisation, the packing, the one upload, the
two kernels, the one download and the scatter.  Host, in the same run on the same box, alternating with the device: the same
call on a host-only handle (the library's host path: the same scalar code compiled by the host compiler, the problems one after
the other on one core).  That comparison is neither g2o nor the reference: no g2o + Eigen build is timed here.  The problems are
marshalled once, outside the timed window.  Median, minimum and maximum of the repetitions are reported; device and host results
are compared bit for bit before anything is timed.  The rounds and the blocks of L of every size are reported with the edges:
blocks - vertices - (edges between free vertices) is the fill."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import essgraph_scenes as sc  # noqa: E402
from orb_slam2_detailed_comments_amd import ORBextractor, _capi, optimizer  # noqa: E402

BATCHES = (1, 4, 16, 64)
SIZES = (100, 400, 1500)
NSCENES = 4           # distinct scenes per size; a call of B problems cycles through them
DEV_REPS = {100: 10, 400: 10, 1500: 5}
HOST_REPS = {(100, 1): 10, (100, 4): 10, (100, 16): 5, (100, 64): 3, (400, 1): 5, (400, 4): 3, (400, 16): 2, (400, 64): 1,
             (1500, 1): 3, (1500, 4): 2, (1500, 16): 1, (1500, 64): 1}


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
    ap.add_argument("--quick", action="store_true", help="the smallest size at B = 1, 4 only (a rehearsal)")
    ap.add_argument("--host-only", action="store_true", help="rehearse the host column where there is no device (times nothing)")
    a = ap.parse_args()
    L = _capi.lib()
    host = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    dev = host if a.host_only else ORBextractor(1000, 1.2, 8, 20, 7)
    lines = ["| keyframes | edges | rounds | blocks of L (fill) | iterations | B | device, ms / problem: median (min - max) | host path, ms / problem: median (min - max) | device call, ms |",
             "|---|---|---|---|---|---|---|---|---|"]
    for n in (SIZES[:1] if a.quick else SIZES):
        scenes = [sc.chain_covis(4000 + k, n, rot_noise=0.005, t_noise=0.02, s_noise=0.005, npoints=10 * n) for k in range(NSCENES)]
        edges = len(scenes[0]["edges"])
        free_edges = int(np.sum((scenes[0]["edges"][:, 0] != 0) & (scenes[0]["edges"][:, 1] != 0)))
        for B in (BATCHES[:2] if a.quick else BATCHES):
            arr_d, hold_d, out_d = optimizer._essgraph_marshal([scenes[k % NSCENES] for k in range(B)])
            arr_h, hold_h, out_h = optimizer._essgraph_marshal([scenes[k % NSCENES] for k in range(B)])
            res_d, res_h = np.zeros(B, _capi.ESSGRAPH_RESULT_DTYPE), np.zeros(B, _capi.ESSGRAPH_RESULT_DTYPE)

            def f_dev():
                _capi.check(L.orbx_optimize_essential_graph_batch(dev.handle, B, C.cast(arr_d, C.c_void_p), _capi.ptr(res_d)))

            def f_host():
                _capi.check(L.orbx_optimize_essential_graph_batch(host.handle, B, C.cast(arr_h, C.c_void_p), _capi.ptr(res_h)))

            f_dev(); f_host()                                   # warm-up, and the check
            assert res_d.tobytes() == res_h.tobytes(), "device and host results differ"
            for d, h in zip(out_d, out_h):
                assert all(x.tobytes() == y.tobytes() for x, y in zip(d, h)), "device and host differ"
            td, th = timed(f_dev, DEV_REPS[n]), timed(f_host, HOST_REPS[(n, B)])
            r = res_d[0]
            lines.append("| %d | %d | %d | %d (%d) | %s | %d | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.2f |" % (
                n, edges, int(r["nrounds"]), int(r["nlblocks"]), int(r["nlblocks"]) - int(r["nactive"]) - free_edges,
                sorted(set(int(x) for x in res_d["iters"])), B, td[1] / B, td[0] / B, td[2] / B, th[1] / B, th[0] / B, th[2] / B, td[1]))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
