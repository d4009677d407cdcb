#!/usr/bin/env python3
"""us per problem of the two batched, device-resident tracking matchers (orbx_search_by_projection_frame_batch_device,
orbx_search_by_projection_mappoints_batch_device) at 1, 64 and 1024 problems per call, next to a loop of the existing single
calls on the SAME inputs (the only path before the batched calls existed) and to the single-thread CPU oracle.

Inputs: 64 consecutive 640x480 frames of the synthetic stream at 1000 features, left on the device as one batch (problem k reads
frame k % 64); the points of problem k are synthesised from the keypoints of the frame before it (the stream moves by (-3, -2)
px per frame), 80 % of them live.  Every call is the raw C entry point with its argument structures built beforehand, timed
with a host clock around call + orbx_synchronize (the single calls synchronise themselves); medians over the repetitions.  Also
reported: the share of live points that take the rescan path (tests/track_model.py on the first problems) and the kernel split
of a 64-problem call from orbx_profile_read.

    python tools/track_rate.py [--json out.json] [--reps 20]
"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oracle
from orb_slam2_detailed_comments_amd import ORBextractor, synth, _capi
from orb_slam2_detailed_comments_amd._capi import ptr

W, H, NF, SIZES = 640, 480, 64, (1, 64, 1024)
BOUNDS = (0.0, float(W), 0.0, float(H))
CAMERA = (500.0, 500.0, 320.0, 240.0)
MB, MBF, ZW = 0.1, 40.0, 2.0


def median_us(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json"); ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    L = _capi.lib()
    ex = ORBextractor(1000, max_batch=NF)
    h = ex.handle
    frames = ex.extract_batch(synth.stream(W, H, NF, stream_id=41))
    cap = max(len(k) for k, _ in frames)
    scale = ex.GetScaleFactors()
    rng = np.random.default_rng(3)
    # the device batch: keypoints (taken as undistorted), descriptors, u_right for half of the features, counts, grids
    keys = np.zeros((NF, cap), _capi.KP_DTYPE); desc = np.zeros((NF, cap, 32), np.uint8)
    ur = np.full((NF, cap), -1.0, np.float32); cnt = np.zeros(NF, np.int32)
    for f, (k, d) in enumerate(frames):
        n = len(k)
        keys[f, :n], desc[f, :n], cnt[f] = k, d, n
        ur[f, :n] = np.where(rng.uniform(size=n) < 0.5, k["x"] - MBF / ZW, -1.0)
    dev = torch.device("cuda", 0)
    d_keys = torch.from_numpy(keys.view(np.uint8).reshape(NF, -1)).to(dev); d_desc = torch.from_numpy(desc).to(dev)
    d_ur = torch.from_numpy(ur).to(dev); d_cnt = torch.from_numpy(cnt).to(dev)
    d_cb = torch.zeros((NF, 64 * 48 + 1), dtype=torch.int32, device=dev); d_it = torch.zeros((NF, cap), dtype=torch.int16, device=dev)
    d_rows = torch.zeros((max(SIZES), cap), dtype=torch.int32, device=dev); d_nm = torch.zeros(max(SIZES), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    b4, cam = np.asarray(BOUNDS, np.float32), np.asarray(CAMERA, np.float32)
    _capi.check(L.orbx_grid_build_device(h, NF, ptr(d_keys), ptr(d_cnt), cap, ptr(b4), ptr(d_cb), ptr(d_it)))
    ex.synchronize()
    devargs = (NF, ptr(d_keys), ptr(d_desc), ptr(d_ur), ptr(d_cnt), cap, ptr(d_cb), ptr(d_it))

    # ---- the problems' host state (64 distinct point sets), as the C structures of both forms
    fx, fy, cx, cy = CAMERA
    eye = np.eye(4, dtype=np.float32); Tlw = eye.copy(); Tlw[2, 3] = 0.3
    keep, host = [], []
    for f in range(NF):
        kp, dp = frames[(f - 1) % NF]
        n = len(kp)
        u = kp["x"] - 3.0 + rng.normal(0, 1.0, n); v = kp["y"] - 2.0 + rng.normal(0, 1.0, n)
        p = dict(keys_un=kp, has=(rng.uniform(size=n) < 0.8).astype(np.uint8),
                 xw=np.stack([(u - cx) / fx * ZW, (v - cy) / fy * ZW, np.full(n, ZW)], 1).astype(np.float32),
                 mpd=np.ascontiguousarray(dp), obs=rng.integers(0, 3, n).astype(np.int32),
                 proj=np.stack([u, v, u - MBF / ZW], 1).astype(np.float32), level=kp["octave"].astype(np.int32),
                 cos=rng.choice([0.99, 0.9999], n).astype(np.float32),
                 fobs=np.where(rng.uniform(size=cap) < 0.2, 2, -1).astype(np.int32))
        host.append(p)
    nprob = max(SIZES)
    FP = (_capi.TrackFrameProblem * nprob)(); PP = (_capi.TrackPointsProblem * nprob)()
    views = []
    for k in range(nprob):
        p = host[k % NF]; f = k % NF
        FP[k].frame, FP[k].th, FP[k].mono = f, 15.0, 0
        FP[k].Tcw[:] = [float(x) for x in eye.reshape(16)]
        lv = FP[k].last
        lv.n = len(p["keys_un"])
        lv.keys_un, lv.has_map_point, lv.world_pos, lv.mp_desc, lv.observations = (p[x].ctypes.data for x in ("keys_un", "has", "xw", "mpd", "obs"))
        lv.Tcw[:] = [float(x) for x in Tlw.reshape(16)]
        PP[k].frame, PP[k].th, PP[k].frame_observations = f, 3.0, p["fobs"].ctypes.data
        mv = PP[k].points
        mv.n = len(p["keys_un"])
        mv.in_view, mv.proj, mv.level, mv.view_cos, mv.desc, mv.observations = (p[x].ctypes.data for x in ("has", "proj", "level", "cos", "mpd", "obs"))
        if k < NF:   # the single calls' views of the same problem
            n = int(cnt[f])
            fv = _capi.FrameView()
            hk, hd, hu = np.ascontiguousarray(keys[f, :n]), np.ascontiguousarray(desc[f, :n]), np.ascontiguousarray(ur[f, :n])
            keep += [hk, hd, hu]
            fv.keys_un, fv.desc, fv.u_right, fv.n = hk.ctypes.data, hd.ctypes.data, hu.ctypes.data, n
            fv.Tcw[:] = [float(x) for x in eye.reshape(16)]
            fv.fx, fv.fy, fv.cx, fv.cy = CAMERA
            fv.min_x, fv.max_x, fv.min_y, fv.max_y = BOUNDS
            fv.mb, fv.mbf = MB, MBF
            views.append((fv, hk, hd, hu))
    out = np.zeros(cap, np.int32); nm = C.c_int(0)

    def batch_ff(K):
        _capi.check(L.orbx_search_by_projection_frame_batch_device(h, K, FP, *devargs, ptr(cam), ptr(b4), MB, MBF, 1, ptr(d_rows), ptr(d_nm)))
        ex.synchronize()

    def batch_mp(K):
        _capi.check(L.orbx_search_by_projection_mappoints_batch_device(h, K, PP, *devargs, ptr(b4), 0.8, ptr(d_rows), ptr(d_nm)))
        ex.synchronize()

    def single_ff(K):
        for k in range(K):
            _capi.check(L.orbx_search_by_projection_frame(h, C.byref(views[k % NF][0]), C.byref(FP[k].last), 15.0, 0, 1, ptr(out), C.byref(nm)))

    def single_mp(K):
        for k in range(K):
            _capi.check(L.orbx_search_by_projection_mappoints(h, C.byref(views[k % NF][0]), ptr(host[k % NF]["fobs"]), C.byref(PP[k].points),
                                                              3.0, 0.8, ptr(out), C.byref(nm)))

    def oracle_ff(K):
        for k in range(K):
            p, (fv, hk, hd, hu) = host[k % NF], views[k % NF]
            oracle.search_by_projection_ff(hk, hd, hu, eye, CAMERA, BOUNDS, MB, MBF, scale, p["keys_un"], p["has"], p["xw"], p["mpd"],
                                           p["obs"], Tlw, 15.0, 0, True, oracle.FP_GCC_FMA)

    def oracle_mp(K):
        for k in range(K):
            p, (fv, hk, hd, hu) = host[k % NF], views[k % NF]
            oracle.search_by_projection_mp(hk, hd, hu, p["fobs"][:len(hk)], BOUNDS, scale, p["has"], p["proj"], p["level"], p["cos"],
                                           p["mpd"], p["obs"], 3.0, 0.8)

    # the batched results are the single calls' (checked on the first 64 problems before anything is timed)
    for name, bfn, sfn in (("frame", batch_ff, single_ff), ("mappoints", batch_mp, single_mp)):
        bfn(NF)
        rows, nms = d_rows.cpu().numpy(), d_nm.cpu().numpy()
        for k in range(NF):
            sfn_one = (lambda: L.orbx_search_by_projection_frame(h, C.byref(views[k][0]), C.byref(FP[k].last), 15.0, 0, 1, ptr(out), C.byref(nm))) \
                if name == "frame" else (lambda: L.orbx_search_by_projection_mappoints(h, C.byref(views[k][0]), ptr(host[k]["fobs"]),
                                                                                       C.byref(PP[k].points), 3.0, 0.8, ptr(out), C.byref(nm)))
            _capi.check(sfn_one())
            n = int(cnt[k])
            assert nm.value == nms[k] and np.array_equal(out[:n], rows[k, :n]), (name, k)

    res = dict(frames=f"{W}x{H}", features=int(cnt.mean()), live_points=float(np.mean([p["has"].sum() for p in host])), reps=a.reps, rows=[])
    for name, bfn, sfn, ofn in (("frame", batch_ff, single_ff, oracle_ff), ("mappoints", batch_mp, single_mp, oracle_mp)):
        cpu = median_us(lambda: ofn(8), 3) / 8
        for K in SIZES:
            reps = max(3, a.reps // (1 + K // 256))
            b = median_us(lambda: bfn(K), reps) / K
            s = median_us(lambda: sfn(K), reps) / K
            b2 = median_us(lambda: bfn(K), reps) / K          # the same command again, alternating: the spread
            s2 = median_us(lambda: sfn(K), reps) / K
            row = dict(policy=name, problems=K, batch_us_per_problem=round(b, 2), batch_again=round(b2, 2),
                       single_loop_us_per_problem=round(s, 2), single_again=round(s2, 2), cpu_oracle_us_per_problem=round(cpu, 1))
            res["rows"].append(row)
            print(row, flush=True)
    # ---- kernel split of a 64-problem call (events on the handle's stream; a run of its own, after the timings)
    ex.profile_enable((1 << 7) | (1 << 8))
    for name, bfn in (("frame", batch_ff), ("mappoints", batch_mp)):
        ex.profile_read(True)
        for _ in range(10):
            bfn(64)
        pr = ex.profile_read(True)   # {kernel id name: (ms, scopes)}: the candidate kernel is timed as k_match, the others as misc
        res[f"split_{name}_64"] = dict(k_track_cand_us=round(pr["k_match"][0] * 1e3 / 10, 1),
                                       project_and_select_us=round(pr["misc"][0] * 1e3 / 10, 1), scopes=[pr["k_match"][1], pr["misc"][1]])
        print(name, res[f"split_{name}_64"], flush=True)
    ex.profile_enable(0)
    # ---- rescan share (the model of tests/track_model.py on the first 4 problems of each policy)
    import track_model as tm
    tm.BOUNDS, tm.CAMERA, tm.MB, tm.MBF = BOUNDS, CAMERA, MB, MBF
    sh = dict(frame=[0, 0], mappoints=[0, 0])
    for k in range(4):
        p, (fv, hk, hd, hu) = host[k], views[k]
        fr = dict(keys=hk, desc=hd, u_right=hu)
        st = tm.model_ff(fr, dict(th=np.float32(15.0), mono=0, Tcw=eye, Tlw=Tlw, keys_un=p["keys_un"], has_map_point=p["has"],
                                  world_pos=p["xw"], mp_desc=p["mpd"], observations=p["obs"]), True, scale)[2]
        sh["frame"][0] += st["rescans"]; sh["frame"][1] += st["live"]
        st = tm.model_mp(fr, dict(th=np.float32(3.0), frame_observations=p["fobs"], in_view=p["has"], proj=p["proj"], level=p["level"],
                                  view_cos=p["cos"], mp_desc=p["mpd"], observations=p["obs"]), 0.8, scale)[2]
        sh["mappoints"][0] += st["rescans"]; sh["mappoints"][1] += st["live"]
    res["rescan_share"] = {k: round(v[0] / max(v[1], 1), 3) for k, v in sh.items()}
    print("rescan share of the points that reach the selection:", res["rescan_share"], flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
