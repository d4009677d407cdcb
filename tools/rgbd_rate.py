#!/usr/bin/env python3
"""Rates of the RGB-D Frame path (k_rgbd: Frame::ComputeStereoFromRGBD fused with the undistortion) at TUM RGB-D settings:
640x480 RGB8 frames, u16 depth (DepthMapFactor 5000), five distortion coefficients and bf 40 (Examples/RGB-D/TUM1.yaml).

  device  the device-resident 1024-frame step, RGB-D (extract + orbx_rgbd_depth_device) against mono (extract +
          orbx_undistort_keypoints_device) on the same frames, interleaved in one process
  host    host-fed calls of 256 and 1024 frames from page-locked memory (chunks of 64): orbx_extract_rgbd_batch with the depth
          uploaded and read in place (ORBX_RGBD_DEPTH), next to the colour-only orbx_extract_batch; interleaved

    python tools/rgbd_rate.py [device] [host] [--reps R]
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from orb_slam2_detailed_comments_amd import ORBextractor, synth, depth_map_factor, _capi

W, H = 640, 480
K = np.array((517.306408, 516.469215, 318.643040, 255.313989), np.float32)
D = np.array((0.262383, -0.953104, -0.005358, 0.002628, 1.163314), np.float32)
MBF = 40.0
SCALE = depth_map_factor(5000.0)
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5


def frames(n):
    """n RGB frames + u16 depth: 16 distinct scenes, rolled so that no two frames of a batch are the same bytes"""
    g = synth.stream(W, H, 16, stream_id=900)
    dep = synth.depth_stream(W, H, 16, stream_id=900)
    rgb = np.stack([g, 255 - g, np.roll(g, 3, axis=2)], axis=-1)
    roll = lambda a, i: a if i < 16 else np.roll(a, (5 * i % H, 11 * i % W), axis=(0, 1))
    return (np.stack([roll(rgb[i % 16], i) for i in range(n)]), np.stack([roll(dep[i % 16], i) for i in range(n)]))


def device(B=1024, steps=10):
    import torch
    dev = torch.device("cuda:0")
    rgb, dep = frames(B)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=B, device=0)
    ex.set_input_format(_capi.FMT_RGB8)
    L = _capi.lib()
    cap = ex.max_keypoints(W, H)
    d_img = torch.from_numpy(rgb).to(dev); d_dep = torch.from_numpy(dep).to(dev)
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device=dev)
    kps, kun, desc = z(B, cap * 28), z(B, cap * 28), z(B, cap * 32)
    cnt, stat = z(B, dt=torch.int32), z(B, dt=torch.int32)
    ur, dp = z(B, cap, dt=torch.float32), z(B, cap, dt=torch.float32)
    P = _capi.ptr
    torch.cuda.synchronize()

    def mono():
        ex.extract_batch_device(d_img, B, W, H, 3 * W, 3 * W * H, kps, desc, cnt, stat, cap)
        _capi.check(L.orbx_undistort_keypoints_device(ex.handle, B, P(kps), P(cnt), cap, P(K), P(D), 5, P(kun)))

    def rgbd():
        ex.extract_batch_device(d_img, B, W, H, 3 * W, 3 * W * H, kps, desc, cnt, stat, cap)
        ex.rgbd_depth_device(B, kps, cnt, cap, K, D, d_dep, _capi.DEPTH_U16, W, H, 2 * W, 2 * W * H, SCALE, MBF, kun, ur, dp)

    def block(fn):
        ex.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            fn()
        ex.synchronize()
        return (time.perf_counter() - t) / steps * 1e3

    for fn in (mono, rgbd, mono, rgbd):
        block(fn)
    tm, tr = [], []
    for _ in range(REPS):
        tm.append(block(mono)); tr.append(block(rgbd))
    with_depth = int((dp.cpu().numpy() > 0).sum()); nk = int(cnt.sum().item())
    mm, mr = float(np.median(tm)), float(np.median(tr))
    print(f"device-resident step, {B} frames (RGB8 640x480, 1000 features; {steps} steps per block, {REPS} interleaved blocks):")
    print(f"  mono  (extract + undistort)        {mm:7.3f} ms  [{min(tm):.3f} .. {max(tm):.3f}]  {B / mm * 1e3:8.0f} frames/s")
    print(f"  RGB-D (extract + k_rgbd, u16)      {mr:7.3f} ms  [{min(tr):.3f} .. {max(tr):.3f}]  {B / mr * 1e3:8.0f} frames/s")
    print(f"  difference {mr - mm:+.3f} ms per step ({(mr - mm) / mm * 100:+.2f} %); {nk} keypoints, {with_depth} with depth")
    sys.stdout.flush()


def host(sizes=(256, 1024), mb=64):
    rgb_all, dep_all = frames(max(sizes))
    L = _capi.lib()
    P = _capi.ptr
    for N in sizes:
        ex = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=mb, device=0)
        ex.set_input_format(_capi.FMT_RGB8)
        cap = ex.max_keypoints(W, H)
        keep = [_capi.PinnedArray((N, H, W, 3)), _capi.PinnedArray((N, H, W), np.uint16),
                _capi.PinnedArray((N, cap), _capi.KP_DTYPE), _capi.PinnedArray((N, cap), _capi.KP_DTYPE),
                _capi.PinnedArray((N, cap, 32)), _capi.PinnedArray((N,), np.int32),
                _capi.PinnedArray((N, cap), np.float32), _capi.PinnedArray((N, cap), np.float32)]
        img, dep, kps, kun, desc, cnt, ur, dp = (k.array for k in keep)
        img[...] = rgb_all[:N]; dep[...] = dep_all[:N]

        def colour():
            _capi.check(L.orbx_extract_batch(ex.handle, N, P(img), W, H, 3 * W, 3 * W * H, P(kps), P(desc), P(cnt), cap))

        def rgbd(mode):
            def run():
                os.environ["ORBX_RGBD_DEPTH"] = mode
                _capi.check(L.orbx_extract_rgbd_batch(ex.handle, N, P(img), W, H, 3 * W, 3 * W * H, P(dep), _capi.DEPTH_U16, 2 * W,
                                                      2 * W * H, SCALE, P(K), P(D), 5, MBF, P(kps), P(kun), P(desc), P(cnt), P(ur),
                                                      P(dp), cap))
            return run

        variants = [("colour only (orbx_extract_batch)", colour), ("RGB-D, depth uploaded", rgbd("upload")),
                    ("RGB-D, depth read in place", rgbd("inplace"))]
        calls = 4 if N <= 256 else 2
        for _, fn in variants:
            fn(); fn()
        times = {name: [] for name, _ in variants}
        for _ in range(REPS):
            for name, fn in variants:
                t = time.perf_counter()
                for _ in range(calls):
                    fn()
                times[name].append((time.perf_counter() - t) / calls)
        print(f"host-fed, {N} frames per call, chunks of {mb}, page-locked inputs and outputs ({REPS} interleaved rounds of {calls} calls):")
        for name, _ in variants:
            ts = times[name]
            print(f"  {name:36s} {N / np.median(ts):8.0f} frames/s  [{N / max(ts):.0f} .. {N / min(ts):.0f}]  {np.median(ts) * 1e3:7.2f} ms per call")
        sys.stdout.flush()
        os.environ.pop("ORBX_RGBD_DEPTH", None)
        del keep, img, dep, kps, kun, desc, cnt, ur, dp
        ex.close()


if __name__ == "__main__":
    which = [a for a in sys.argv[1:] if a in ("device", "host")] or ["device", "host"]
    if "device" in which:
        device()
    if "host" in which:
        host()
