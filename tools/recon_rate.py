"""Microseconds per initialisation attempt of the batched ReconstructH / ReconstructF on the device against the library's own
host path, and of the fused Initialize call against the two calls it replaces.

    python tools/recon_rate.py [--out <table.md>] [--quick]

Stand-alone: orbx_init_reconstruct_batch_create, one call of P = 1, 16, 64, 256 problems (the outstanding initialisation
attempts of a tracker that feeds many streams), every problem with n = 100, 300 or 1000 matches of which a quarter are displaced
and masked out, model H (a plane, 8 pose hypotheses) or F (a general scene, 4); the matrix is formed from the planted motion.  The
time is a host clock around the C call, which returns after its one download, so it contains validation, the packing, the upload,
the three kernels, the download, the scatter into the batch, acos and the accept / reject arithmetic.  The ctypes problem array is
built before the clock starts.  Host, in the same run on the same box, alternating with the device: the same call on a host-only
handle (the library's host path: the same scalar code compiled by the host compiler, the problems one after the other on one
core).  That host path is neither the reference nor OpenCV.

Fused: orbx_initialize_batch_create against orbx_init_ransac_batch_create followed by orbx_init_reconstruct_batch_create fed with
its result (the read-back of the winning matrix and mask and the marshalling of the second call are inside the clock: that is what
the fused call removes), both on the device, 200 iterations and both models per problem, general scenes and planes in turn.

Median, minimum and maximum of the repetitions (100 / 30 / 10 / 5 for P = 1 / 16 / 64 / 256) are reported; device and host
results are compared bit for bit before anything is timed.  No threshold is set: the tables say what was measured."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import init_scenes as isc  # noqa: E402
import recon_model as rm  # noqa: E402
import recon_scenes as rs  # noqa: E402
from orb_slam2_detailed_comments_amd import (InitializerRansac, InitializerReconstruct, ORBextractor, _capi,  # noqa: E402
                                             initialize_batch)

SIZES = (1, 16, 64, 256)
NS = (100, 300, 1000)
REPS = {1: 100, 16: 30, 64: 10, 256: 5}


def marshal(problems):
    arr = (_capi.ReconProblem * len(problems))()
    keep = []
    for a, p in zip(arr, problems):
        k1, k2 = np.ascontiguousarray(p["keys1"], np.float32), np.ascontiguousarray(p["keys2"], np.float32)
        m, inl = np.ascontiguousarray(p["matches"], np.int32), np.ascontiguousarray(p["inliers"]).astype(np.uint8)
        keep += [k1, k2, m, inl]
        a.n1, a.n2, a.n = len(k1), len(k2), len(m)
        a.keys1, a.keys2, a.matches, a.inliers = k1.ctypes.data, k2.ctypes.data, m.ctypes.data, inl.ctypes.data
        a.model, a.sigma, a.min_parallax, a.min_triangulated = int(p["model"]), 1.0, 1.0, 50
        a.M[:] = [float(v) for v in np.asarray(p["M"], np.float32).reshape(9)]
        a.K[:] = rs.K4
    return arr, keep


def create(L, handle, arr, n):
    b = C.c_void_p()
    _capi.check(L.orbx_init_reconstruct_batch_create(handle, n, C.cast(arr, C.c_void_p), C.byref(b)))
    return b


def everything(rc, k, nh):
    r = rc.result(k)
    out = [np.array([r["ok"], r["chosen"], r["N"]]), rs.bits(r["R21"]), rs.bits(r["t21"]), r["status"], rs.bits(r["points"])]
    for i in range(nh):
        h = rc.hypothesis(k, i)
        out += [rs.bits(h["R"]), rs.bits(h["t"]), rs.bits(h["n"]), np.array([h["nGood"], h["valid"]]), rs.bits(h["cosine"]),
                rs.bits(h["parallax"])]
    return out


def line(tag, n, P, reps, ta, tb, names):
    print(f"{tag} n {n:4d}  P {P:3d}  reps {reps:4d}  {names[0]} {np.median(ta):9.1f} ({ta.min():.1f} - {ta.max():.1f}) us/attempt   "
          f"{names[1]} {np.median(tb):9.1f} ({tb.min():.1f} - {tb.max():.1f})   x{np.median(tb) / np.median(ta):.2f}   "
          f"{names[0]} call {np.median(ta) * P / 1e3:.3f} ms", flush=True)


def table(f, title, rows, names):
    f.write(f"\n{title}\n\n| model | n | P | repetitions | {names[0]}, us / attempt: median (min - max) | {names[1]}, us / attempt: median (min - max) | "
            f"{names[1]} / {names[0]} | {names[0]} call, ms |\n|---|---|---|---|---|---|---|---|\n")
    for tag, n, P, reps, ta, tb in rows:
        f.write(f"| {tag} | {n} | {P} | {reps} | {np.median(ta):.1f} ({ta.min():.1f} - {ta.max():.1f}) | {np.median(tb):.1f} ({tb.min():.1f} - {tb.max():.1f}) | "
                f"{np.median(tb) / np.median(ta):.2f} | {np.median(ta) * P / 1e3:.3f} |\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a fifth of the repetitions")
    args = ap.parse_args()
    L = _capi.lib()
    dev = ORBextractor(1000, 1.2, 8, 20, 7)
    host = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    plane = dict(R=isc.rot([0.2, 1.0, 0.1], -20.0), t=[2.0, 0.0, 0.5])
    alone, fused = [], []
    for tag, kind, kw in (("H", "plane", plane), ("F", "general", {})):
        for n in NS:
            base = [rs.scene(8000 + n + k, n, kind, outliers=0.25, extra1=n // 2, extra2=n // 2, **kw) for k in range(8)]
            for P in SIZES:
                problems = [base[k % 8] for k in range(P)]      # the same eight scenes over and over: the work per attempt is what counts
                arr, keep = marshal(problems)
                if P <= 16:
                    rd, rh = InitializerReconstruct(dev, problems), InitializerReconstruct(host, problems)
                    for k in range(P):
                        assert all(np.array_equal(x, y) for x, y in zip(everything(rd, k, 8 if tag == "H" else 4),
                                                                        everything(rh, k, 8 if tag == "H" else 4))), "device and host path differ"
                    assert rd.result(0)["ok"]
                    rd.close(), rh.close()
                reps = max(3, REPS[P] // (5 if args.quick else 1))
                for _ in range(2):                             # warm-up of this shape on both paths
                    L.orbx_recon_batch_destroy(create(L, dev.handle, arr, P)); L.orbx_recon_batch_destroy(create(L, host.handle, arr, P))
                td, th = [], []
                for _ in range(reps):
                    for handle, t in ((dev.handle, td), (host.handle, th)):
                        t0 = time.perf_counter()
                        b = create(L, handle, arr, P)
                        t.append(time.perf_counter() - t0)
                        L.orbx_recon_batch_destroy(b)
                td, th = np.array(td) * 1e6 / P, np.array(th) * 1e6 / P
                alone.append((tag, n, P, reps, td, th))
                line(tag, n, P, reps, td, th, ("device", "host"))
    for n in NS:
        base = [isc.make(9000 + n + k, n, ("general", "plane")[k % 2], iterations=200, extra1=n // 2, extra2=n // 2) for k in range(8)]
        for P in SIZES:
            problems = [base[k % 8] for k in range(P)]
            cams = [rs.camera() for _ in problems]

            def two_calls():
                rb = InitializerRansac(dev, problems)
                rc = InitializerReconstruct(dev, [rs.from_ransac(p, rb.result(k), cams[k]) for k, p in enumerate(problems)])
                return rb, rc

            def one_call():
                return initialize_batch(dev, problems, cams)

            if P <= 16:
                (a, b), (c, d) = one_call(), two_calls()
                for k in range(P):
                    nh = 8 if a.result(k)["model"] == rm.H else 4
                    assert all(np.array_equal(x, y) for x, y in zip(everything(b, k, nh), everything(d, k, nh))), "fused and two calls differ"
                for x in (a, b, c, d):
                    x.close()
            reps = max(3, REPS[P] // (5 if args.quick else 1))
            tf, t2 = [], []
            for i in range(reps + 2):                           # the first two rounds are the warm-up
                for fn, t in ((one_call, tf), (two_calls, t2)):
                    t0 = time.perf_counter()
                    x, y = fn()
                    dt = time.perf_counter() - t0
                    x.close(), y.close()
                    if i >= 2:
                        t.append(dt)
            tf, t2 = np.array(tf) * 1e6 / P, np.array(t2) * 1e6 / P
            fused.append(("H+F", n, P, reps, tf, t2))
            line("fused", n, P, reps, tf, t2, ("fused", "two calls"))
    if args.out:
        with open(args.out, "w") as f:
            table(f, "Stand-alone call: device against the host path", alone, ("device", "host path"))
            table(f, "Fused call against the two calls it replaces, both on the device (Python wrappers inside the clock on both sides)", fused,
                  ("fused", "two calls"))
    dev.close(), host.close()


if __name__ == "__main__":
    main()
