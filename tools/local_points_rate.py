#!/usr/bin/env python3
"""Time per call and uploaded bytes of Tracking::SearchLocalPoints on the device (orbx_search_local_points_batch_device: the
frustum stage and the matcher in one call, ONE shared pool uploaded once) next to the route it replaces: Frame::isInFrustum +
PredictScale on the host -- here a numpy pass vectorised over the pool, per problem -- and then
orbx_search_by_projection_mappoints_batch_device, which takes every problem's own copy of every point's query and descriptor.

Shapes: 64 problems of one 64-frame device batch (640x480 synthetic stream, 1000 features) against one 2000-point pool, and 1
problem.  The pool holds the keypoints of frames 0 and 32 lifted to depth 2 m; problem k looks at frame k from a pose that
follows the stream's motion, so that a part of the pool projects onto its features and the rest leaves the frustum through
one gate or another.  Both routes are timed with a host clock around everything a caller would run per batch (host frustum
where there is one, argument structures, the call, orbx_synchronize); medians over the repetitions, each command twice.  The
uploaded bytes are counted from the staging layouts of csrc/orbx_track_pack.cpp (256-byte padded sections).

    python tools/local_points_rate.py [--md profiles/local_points_rate.md] [--reps 20]
"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from orb_slam2_detailed_comments_amd import ORBextractor, synth, _capi
from orb_slam2_detailed_comments_amd._capi import ptr

W, H, NF, M = 640, 480, 64, 2000
BOUNDS = (0.0, float(W), 0.0, float(H))
CAMERA = (500.0, 500.0, 320.0, 240.0)
MBF, ZW, TH, NNRATIO = 40.0, 2.0, 3.0, 0.8
F32 = np.float32


def median_us(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6


def pad256(b):
    return (b + 255) & ~255


def staged_local(P, npool, nq, cap):
    return (pad256(P * 64) + pad256(P * 32) + pad256(npool * 36) + pad256(npool * 32) + pad256(nq * 4) + pad256(nq) +
            pad256(P * ((cap + 31) // 32) * 4))


def staged_points(P, nq, cap):
    return pad256(P * 64) + pad256(nq * 40) + pad256(nq * 32) + pad256(P * ((cap + 31) // 32) * 4)


def host_frustum(T, Ow, pool, scale, log_sf, nlevels):
    """isInFrustum + PredictScale over the whole pool in float32 numpy: what a caller of the map-point call runs per frame"""
    fx, fy, cx, cy = (F32(v) for v in CAMERA)
    P = pool["world_pos"]
    Pc = P @ T[:3, :3].T + T[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        invz = F32(1.0) / Pc[:, 2]
        u = fx * Pc[:, 0] * invz + cx
        v = fy * Pc[:, 1] * invz + cy
        PO = P - Ow
        dist = np.sqrt((PO.astype(np.float64) ** 2).sum(1)).astype(F32)
        cos = ((PO.astype(np.float64) * pool["normal"]).sum(1) / dist).astype(F32)
        ok = ~(Pc[:, 2] < 0) & ~(u < BOUNDS[0]) & ~(u > BOUNDS[1]) & ~(v < BOUNDS[2]) & ~(v > BOUNDS[3])
        ok &= ~(dist < F32(0.8) * pool["min_distance"]) & ~(dist > F32(1.2) * pool["max_distance"]) & ~(cos < F32(0.5))
        lvl = np.ceil(np.log(pool["max_distance"] / dist) / log_sf)
        lvl = np.clip(np.nan_to_num(lvl, nan=0.0, posinf=nlevels - 1, neginf=0.0), 0, nlevels - 1).astype(np.int32)
    proj = np.stack([u, v, u - F32(MBF) * invz], 1).astype(F32)
    return ok.astype(np.uint8), proj, lvl, cos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md"); ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    L = _capi.lib()
    ex = ORBextractor(1000, max_batch=NF)
    h = ex.handle
    frames = ex.extract_batch(synth.stream(W, H, NF, stream_id=41))
    cap = max(len(k) for k, _ in frames)
    scale = ex.GetScaleFactors()
    nlevels = L.orbx_get_levels(h)
    log_sf = F32(np.log(F32(L.orbx_get_scale_factor(h))))
    rng = np.random.default_rng(3)
    keys = np.zeros((NF, cap), _capi.KP_DTYPE); desc = np.zeros((NF, cap, 32), np.uint8)
    ur = np.full((NF, cap), -1.0, F32); cnt = np.zeros(NF, np.int32)
    for f, (k, d) in enumerate(frames):
        n = len(k)
        keys[f, :n], desc[f, :n], cnt[f] = k, d, n
        ur[f, :n] = np.where(rng.uniform(size=n) < 0.5, k["x"] - MBF / ZW, -1.0)
    dev = torch.device("cuda", 0)
    d_keys = torch.from_numpy(keys.view(np.uint8).reshape(NF, -1)).to(dev); d_desc = torch.from_numpy(desc).to(dev)
    d_ur = torch.from_numpy(ur).to(dev); d_cnt = torch.from_numpy(cnt).to(dev)
    d_cb = torch.zeros((NF, 64 * 48 + 1), dtype=torch.int32, device=dev); d_it = torch.zeros((NF, cap), dtype=torch.int16, device=dev)
    d_rows = torch.zeros((NF, cap), dtype=torch.int32, device=dev); d_nm = torch.zeros(NF, dtype=torch.int32, device=dev)
    d_rows2 = torch.zeros((NF, cap), dtype=torch.int32, device=dev); d_nm2 = torch.zeros(NF, dtype=torch.int32, device=dev)
    d_iv = torch.zeros(NF * M, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    b4, cam = np.asarray(BOUNDS, F32), np.asarray(CAMERA, F32)
    _capi.check(L.orbx_grid_build_device(h, NF, ptr(d_keys), ptr(d_cnt), cap, ptr(b4), ptr(d_cb), ptr(d_it)))
    ex.synchronize()
    devargs = (NF, ptr(d_keys), ptr(d_desc), ptr(d_ur), ptr(d_cnt), cap, ptr(d_cb), ptr(d_it))

    # ---- the pool: the keypoints of frames 0 and 32 at depth ZW, seen from the identity pose of their frame
    fx, fy, cx, cy = CAMERA
    parts = []
    for f in (0, 32):
        k, d = frames[f]
        n = min(len(k), M // 2)
        xw = np.stack([(k["x"][:n] + 3.0 * f - cx) / fx * ZW, (k["y"][:n] + 2.0 * f - cy) / fy * ZW, np.full(n, ZW)], 1)
        parts.append((xw, d[:n], k["octave"][:n]))
    xw = np.concatenate([p[0] for p in parts]).astype(F32)
    npool = len(xw)
    dist0 = np.linalg.norm(xw, axis=1)
    octv = np.concatenate([p[2] for p in parts])
    maxd = (dist0 * 1.2 ** (octv - 0.5)).astype(F32)
    pool = dict(world_pos=xw, normal=np.ascontiguousarray(xw / dist0[:, None], F32), min_distance=(maxd / F32(1.2 ** 7)).astype(F32), max_distance=maxd,
                desc=np.ascontiguousarray(np.concatenate([p[1] for p in parts])), observations=rng.integers(0, 3, npool).astype(np.int32))
    mv = _capi.LocalMapView()
    mv.n = npool
    mv.world_pos, mv.normal, mv.min_distance, mv.max_distance, mv.desc, mv.observations = (
        pool[k].ctypes.data for k in ("world_pos", "normal", "min_distance", "max_distance", "desc", "observations"))
    # ---- the problems: frame k from the pose that follows the stream (-3, -2 px per frame at depth ZW)
    fobs = [np.where(rng.uniform(size=cap) < 0.2, 2, -1).astype(np.int32) for _ in range(NF)]
    poses, centres = [], []
    LP = (_capi.TrackLocalProblem * NF)()
    for k in range(NF):
        T = np.eye(4, dtype=F32)
        T[0, 3], T[1, 3] = -3.0 * k / fx * ZW, -2.0 * k / fy * ZW
        Ow = (-T[:3, 3]).astype(F32)
        poses.append(T); centres.append(Ow)
        LP[k].frame, LP[k].th, LP[k].viewing_cos_limit, LP[k].npoints = k, TH, 0.5, npool
        LP[k].Tcw[:] = [float(x) for x in T.reshape(16)]
        LP[k].Ow[:] = [float(x) for x in Ow]
        LP[k].frame_observations = fobs[k].ctypes.data

    def new_route(K):
        _capi.check(L.orbx_search_local_points_batch_device(h, K, LP, C.byref(mv), *devargs, ptr(cam), ptr(b4), MBF, NNRATIO, ptr(d_rows),
                                                            ptr(d_nm), ptr(d_iv), None))
        ex.synchronize()

    keep = {}

    def old_route(K):
        PP = (_capi.TrackPointsProblem * K)()
        hold = []
        for k in range(K):
            iv, proj, lvl, cos = host_frustum(poses[k], centres[k], pool, scale, log_sf, nlevels)
            hold.append((iv, proj, lvl, cos))
            PP[k].frame, PP[k].th, PP[k].frame_observations = k, TH, fobs[k].ctypes.data
            pv = PP[k].points
            pv.n = npool
            pv.in_view, pv.proj, pv.level, pv.view_cos = iv.ctypes.data, proj.ctypes.data, lvl.ctypes.data, cos.ctypes.data
            pv.desc, pv.observations = pool["desc"].ctypes.data, pool["observations"].ctypes.data
        _capi.check(L.orbx_search_by_projection_mappoints_batch_device(h, K, PP, *devargs, ptr(b4), NNRATIO, ptr(d_rows2), ptr(d_nm2)))
        ex.synchronize()
        keep["hold"] = hold

    def old_device_part(K):
        """the map-point call alone on fields computed beforehand: what the host frustum adds is old_route minus this"""
        _capi.check(L.orbx_search_by_projection_mappoints_batch_device(h, K, keep["PP"], *devargs, ptr(b4), NNRATIO, ptr(d_rows2), ptr(d_nm2)))
        ex.synchronize()

    # the two routes find the same matches wherever numpy's logarithm puts a point on the level libm does
    new_route(NF); old_route(NF)
    nm_new, nm_old = d_nm.cpu().numpy(), d_nm2.cpu().numpy()
    iv_new = d_iv.cpu().numpy()[:NF * npool].reshape(NF, npool)
    iv_old = np.stack([hd[0] for hd in keep["hold"]])
    same_rows = int((d_rows.cpu().numpy() == d_rows2.cpu().numpy()).all(1).sum())
    PP = (_capi.TrackPointsProblem * NF)()
    for k, (iv, proj, lvl, cos) in enumerate(keep["hold"]):
        PP[k].frame, PP[k].th, PP[k].frame_observations = k, TH, fobs[k].ctypes.data
        pv = PP[k].points
        pv.n = npool
        pv.in_view, pv.proj, pv.level, pv.view_cos = iv.ctypes.data, proj.ctypes.data, lvl.ctypes.data, cos.ctypes.data
        pv.desc, pv.observations = pool["desc"].ctypes.data, pool["observations"].ctypes.data
    keep["PP"], keep["fields"] = PP, list(keep["hold"])

    lines = ["# SearchLocalPoints on the device: time per call and uploaded bytes", "",
             f"Written by `tools/local_points_rate.py` ({a.reps} repetitions, medians, every command twice).  {NF} frames of {W}x{H}, "
             f"{int(cnt.mean())} features each, cap {cap}; one pool of {npool} points; th {TH}, nnratio {NNRATIO}.", "",
             f"In view: {iv_new.mean() * 100:.1f} % of the (problem, point) pairs on the device, {iv_old.mean() * 100:.1f} % in the numpy pass; "
             f"matches per problem {nm_new.mean():.1f} (device route) and {nm_old.mean():.1f} (host frustum route); "
             f"{same_rows} of {NF} output rows identical (the numpy pass takes its levels from np.log, not from libm).", "",
             "| problems | route | us per call | again | us per problem | uploaded bytes per call |", "|---|---|---|---|---|---|"]
    for K in (NF, 1):
        rows = (("device frustum + matcher (orbx_search_local_points_batch_device)", lambda: new_route(K), staged_local(K, npool, K * npool, cap)),
                ("numpy frustum + orbx_search_by_projection_mappoints_batch_device", lambda: old_route(K), staged_points(K, K * npool, cap)),
                ("... of which the map-point call alone", lambda: old_device_part(K), staged_points(K, K * npool, cap)))
        for name, fn, nbytes in rows:
            t1 = median_us(fn, a.reps); t2 = median_us(fn, a.reps)
            line = f"| {K} | {name} | {t1:.0f} | {t2:.0f} | {min(t1, t2) / K:.1f} | {nbytes} |"
            lines.append(line)
            print(line, flush=True)
    lines += ["", f"Derived sizes for comparison: P*M*72 = {NF * npool * 72} bytes for {NF} problems and {npool * 72} for one; "
                  f"M*(32+36) + P*(M*5+100) = {npool * 68 + NF * (npool * 5 + 100)} and {npool * 68 + npool * 5 + 100}.  The counted values "
                  "add the blocked-feature seeds and the padding of each section to 256 bytes."]
    print("\n".join(lines[:5]))
    if a.md:
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
