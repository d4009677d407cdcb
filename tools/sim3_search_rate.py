"""Microseconds per candidate of the SearchBySim3 stage of one ComputeSim3 round: the batched call against K single calls.

    python tools/sim3_search_rate.py [--out FILE] [--quick] [--host-only]

K = 1, 4, 16, 64 problems share KF1; every keyframe has N = 500, 1000 or 2000 features.  Compared in the same run on the same
box, the alternatives interleaved repetition by repetition:
  (a) the path before orbx_search_by_sim3_batch: K calls of orbx_search_by_sim3 (two synchronous device round trips each, KF1
      uploaded and gridded in each), fed projections that are computed beforehand.  That precomputation -- the pose algebra the
      caller ran per point in compat/ORBmatcher.h -- is timed separately as ONE call of the new host path over the K problems
      (it also runs the selection, so it overstates the algebra) and reported as "(a) + precompute";
  (b) orbx_search_by_sim3_batch on a host-only handle (the library's host path, one core);
  (c) orbx_search_by_sim3_batch on the device.
The time is a host clock around the C calls, which end in the wait for the handle's stream: validation, packing, upload, kernels,
download and scatter are inside.  Arguments are marshalled once, outside the timed window.  Median, minimum and maximum of the
repetitions are reported; (a), (b) and (c) are compared for equal matches before anything is timed.  Scene: KF1 at the identity, K
keyframes a few centimetres and degrees away, points at depth 1 .. 4 with a keypoint within two pixels of each projection in both
keyframes, 70 % of the features holding a point and 10 % of KF1's already matched."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from orb_slam2_detailed_comments_amd import ORBextractor, ORBmatcher, _capi  # noqa: E402
from orb_slam2_detailed_comments_amd.matcher import Sim3SearchCall  # noqa: E402

KS = (1, 4, 16, 64)
NS = (500, 1000, 2000)
REPS = {1: 60, 4: 30, 16: 12, 64: 5}
W, H, FX, CX, CY = 640, 480, 256.0, 320.0, 240.0
F = np.float32


def rodrigues(rng, angle):
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def keyframe(rng, R, t, X, desc, level):
    """the keyframe of pose [R | t] over the world points X: a keypoint within two pixels of every projection"""
    n = len(X)
    c = X @ R.T + t
    keys = np.zeros(n, _capi.KP_DTYPE)
    keys["x"] = np.clip(FX * c[:, 0] / c[:, 2] + CX + rng.uniform(-2, 2, n), 1, W - 8)
    keys["y"] = np.clip(FX * c[:, 1] / c[:, 2] + CY + rng.uniform(-2, 2, n), 1, H - 8)
    keys["octave"] = np.clip(level - rng.integers(0, 2, n), 0, 7)
    keys["class_id"] = -1
    d = desc.copy()
    flip = rng.integers(0, 256, (n, 12))
    for j in range(12):
        d[np.arange(n), flip[:, j] >> 3] ^= (1 << (flip[:, j] & 7)).astype(np.uint8)
    dist = np.linalg.norm(c, axis=1)
    T = np.eye(4, dtype=F); T[:3, :3] = R; T[:3, 3] = t
    dmax = (dist * 1.2 ** (level - 0.5)).astype(F)
    return dict(keys_un=keys, desc=d, Tcw=T, has_point=(rng.uniform(size=n) < 0.7).astype(np.uint8), world_pos=X.astype(F),
                min_distance=(dmax / F(1.2 ** 7)).astype(F), max_distance=dmax, point_desc=desc)


def scene(N, K, seed=0):
    rng = np.random.default_rng(7000 + seed)
    z = rng.uniform(1.0, 4.0, N)
    X = np.stack([(rng.uniform(40, W - 40, N) - CX) / FX * z, (rng.uniform(40, H - 40, N) - CY) / FX * z, z], axis=1)
    desc = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    level = rng.integers(0, 6, N)
    kfs = [keyframe(rng, np.eye(3), np.zeros(3), X, desc, level)]
    probs = []
    for k in range(K):
        R2, t2 = rodrigues(rng, rng.uniform(0.01, 0.05)), rng.uniform(-0.05, 0.05, 3)
        kfs.append(keyframe(rng, R2, t2, X, desc, level))
        # c1 = s12 R12 c2 + t12 with c1 = X, c2 = R2 X + t2 (s12 = 1): R12 = R2^T, t12 = -R2^T t2, a little off
        R12 = (R2.T @ rodrigues(rng, 0.002)).astype(F)
        t12 = (-R2.T @ t2 + rng.uniform(-0.002, 0.002, 3)).astype(F)
        probs.append(dict(kf1=0, kf2=k + 1, s12=1.0, R12=R12, t12=t12, th=7.5, matched1=(rng.uniform(size=N) < 0.1).astype(np.uint8),
                          matched2=(rng.uniform(size=N) < 0.1).astype(np.uint8)))
    return dict(keyframes=kfs, problems=probs, camera4=np.array([FX, FX, CX, CY], F), bounds4=np.array([0, W, 0, H], F))


def single_calls(m, s, dbg):
    """the marshalled K calls of orbx_search_by_sim3 on the projections the debug rows of the new call give"""
    sf = np.ones(8, F)
    for l in range(1, 8):
        sf[l] = F(sf[l - 1] * F(1.2))
    calls, keep = [], []
    for k, p in enumerate(s["problems"]):
        views = []
        for side, kf in ((1, p["kf1"]), (2, p["kf2"])):
            K_ = s["keyframes"][kf]
            views.append(m._target(dict(keys_un=K_["keys_un"], desc=K_["desc"], bounds=tuple(float(b) for b in s["bounds4"]), scale_factors=sf), keep))
        pts = []
        for side, kf in ((1, p["kf1"]), (2, p["kf2"])):
            st = dbg[k]["status%d" % side]
            valid = (st >= _capi.SIM3S_NO_CANDIDATE).astype(np.uint8)
            pts.append(m._points(dict(valid=valid, uv=np.where(valid[:, None] > 0, dbg[k]["uv%d" % side], 0).astype(F),
                                      level=np.where(valid > 0, dbg[k]["level%d" % side], 0).astype(np.int32),
                                      desc=s["keyframes"][kf]["point_desc"]), keep))
        out, n = np.full(views[0].n, -1, np.int32), C.c_int(0)
        calls.append((views[0], views[1], pts[0], pts[1], float(p["th"]), out, n))
    return calls, keep


def stats(t, K):
    return tuple(1e6 * float(f(t)) / K for f in (np.median, np.min, np.max))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal)")
    ap.add_argument("--host-only", action="store_true", help="rehearse the host column where there is no device (times nothing on the device)")
    a = ap.parse_args()
    L = _capi.lib()
    host = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    dev = None if a.host_only else ORBextractor(1000, 1.2, 8, 20, 7)
    m = ORBmatcher(extractor=dev if dev is not None else host)
    fmt = lambda s: "%.1f (%.1f - %.1f)" % s
    lines = ["us per candidate: median (min - max) of the repetitions", "",
             "| N | K | (a) K single calls | (a) + precompute | (b) batch, host path | (c) batch, device | matches / candidate |",
             "|---|---|---|---|---|---|---|"]
    for N in (NS[:1] if a.quick else NS):
        for K in (KS[:2] if a.quick else KS):
            s = scene(N, K)
            counts, matches, dbg = Sim3SearchCall(s["keyframes"], s["problems"], s["camera4"], s["bounds4"], debug=True).run(host)
            call = Sim3SearchCall(s["keyframes"], s["problems"], s["camera4"], s["bounds4"])
            f_host = lambda: call.run_raw(host)
            if dev is None:
                f_host()
                print("rehearsal: N %d K %d matches / candidate %.1f" % (N, K, float(np.mean(counts))), flush=True)
                continue
            singles, keep = single_calls(m, s, dbg)

            def f_single():
                for t1, t2, p12, p21, th, out, n in singles:
                    _capi.check(L.orbx_search_by_sim3(dev.handle, C.byref(t1), C.byref(t2), C.byref(p12), C.byref(p21), th, _capi.ptr(out), C.byref(n)))

            f_dev = lambda: call.run_raw(dev)
            f_dev()
            got = [call.matches[k][:N].copy() for k in range(K)]
            f_single()
            assert all(np.array_equal(got[k], matches[k]) and np.array_equal(singles[k][5][:N], matches[k]) for k in range(K)), "paths differ"
            ts, th_, td = [], [], []
            for _ in range(REPS[K]):
                for f, t in ((f_single, ts), (f_host, th_), (f_dev, td)):
                    t0 = time.perf_counter()
                    f()
                    t.append(time.perf_counter() - t0)
            with_pre = [x + y for x, y in zip(ts, th_)]
            lines.append("| %d | %d | %s | %s | %s | %s | %.1f |" % (N, K, fmt(stats(ts, K)), fmt(stats(with_pre, K)), fmt(stats(th_, K)),
                                                                   fmt(stats(td, K)), float(np.mean(counts))))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
