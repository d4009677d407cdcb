"""Microseconds per frame of the batched Optimizer::PoseOptimization on the device against the library's own host path.

    python tools/pose_rate.py [--out profiles/pose_batch.md] [--quick]

Device: orbx_pose_optimization_batch_device, one call of P = 1, 64, 1024 problems, every problem a frame of its own (device
rows already in place, as the tracking matchers leave them); the time is a host clock around the call and the wait for the
handle's stream, so it contains the packing, the one upload and the kernel.  Host, in the same run on the same box,
alternating with the device: the same call on a host-only handle (the library's host path: the same scalar code compiled by
the host compiler, the problems one after the other on one core).  About 100, 300 and 1000 edges per frame, all monocular and
all stereo; one pixel of noise, 20 % planted outliers, the start pose a few centimetres off.  Median, minimum and maximum of the repetitions (1000 / 30 / 5 for P = 1 / 64 / 1024) are
reported; device and host results are compared bit for bit before anything is timed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pose_scenes as ps  # noqa: E402
from orb_slam2_detailed_comments_amd import ORBextractor, optimizer  # noqa: E402

SIZES = (1, 64, 1024)
EDGES = (100, 300, 1000)
NSCENES = 16          # distinct scenes per shape; a call of P problems cycles through them under distinct start poses


def build(nedges, mode, P, cap):
    scenes = [ps.make(1000 + k, nedges, mode, 1.0, 0.2, nfeat=cap) for k in range(min(NSCENES, P))]
    rng = np.random.default_rng(nedges + P)
    out = []
    for k in range(P):
        s = scenes[k % len(scenes)]
        if k >= len(scenes):
            d = ps.pose(rng.normal(0, 0.01, 3), rng.normal(0, 0.02, 3))
            s = ps.variant(s, Tcw0=(d @ s["Tcw_true"].astype(np.float64)).astype(np.float32))
        out.append(s)
    # frames are shared by the problems that cycle through one scene; pools are per scene
    b = ps.batch(scenes, cap, use_index=False)
    probs, world = [], b["world"]
    point = np.zeros((P, cap), np.int32)
    for k, s in enumerate(out):
        f = k % len(scenes)
        probs.append(dict(frame=f, Tcw=s["Tcw0"]))
        point[k] = b["point"][f]
    return b, probs, point


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
    a = ap.parse_args()
    import torch
    dev = ORBextractor(1000, 1.2, 8, 20, 7)
    host = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    lines = ["| edges | kind | P | device, us / frame: median (min - max) | host path, us / frame: median (min - max) | device call, ms |",
             "|---|---|---|---|---|---|"]
    for nedges in (EDGES[:1] if a.quick else EDGES):
        cap = nedges + nedges // 4
        for mode in ("mono", "stereo"):
            for P in (SIZES[:2] if a.quick else SIZES):
                b, probs, point = build(nedges, mode, P, cap)
                keys8 = b["keys"].view(np.uint8).reshape(b["nframes"], -1)
                hT, ho, hn = np.zeros((P, 16), np.float32), np.zeros((P, cap), np.uint8), np.zeros(P, np.int32)
                dT, do, dn = up(hT), up(ho), up(hn)
                dk, du, dc, dp = up(keys8), up(b["u_right"]), up(b["counts"]), up(point)
                torch.cuda.synchronize()

                def f_dev():
                    optimizer.pose_optimization_batch(dev, probs, b["world"], b["nframes"], dk, du, dc, cap, dp, ps.CAMERA4, ps.MBF,
                                                      ps.INV_SIGMA2, dT, do, dn)
                    dev.synchronize()

                def f_host():
                    optimizer.pose_optimization_batch(host, probs, b["world"], b["nframes"], keys8, b["u_right"], b["counts"], cap, point,
                                                      ps.CAMERA4, ps.MBF, ps.INV_SIGMA2, hT, ho, hn)

                f_dev(); f_host()
                assert np.array_equal(dT.cpu().numpy().view(np.uint32), hT.view(np.uint32)), "device and host poses differ"
                assert np.array_equal(do.cpu().numpy(), ho) and np.array_equal(dn.cpu().numpy(), hn), "device and host flags differ"
                reps = 1000 if P == 1 else 30 if P == 64 else 5          # every window is a good part of a second at least
                td, th = median_pair(f_dev, f_host, reps)
                lines.append("| %d | %s | %d | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.3f |"
                             % (nedges, mode, P, td[1] / P, td[0] / P, td[2] / P, th[1] / P, th[0] / P, th[2] / P, td[1] / 1e3))
                print(lines[-1], "inliers %.0f of %d" % (hn.mean(), nedges), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
