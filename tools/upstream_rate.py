#!/usr/bin/env python3
"""Step time of the device-resident 1024 x 640x480 extraction (1000 features, grey) in the two pyramid modes:

  upstream     ORBX_PYRAMID_UPSTREAM (un-padded levels; always writes level 0 during the call)
  fork-eager   ORBX_PYRAMID_FORK_PADDED with ORBX_LEVEL0_INPLACE=0: the like-for-like path (level 0 written during the call)
  fork         ORBX_PYRAMID_FORK_PADDED as shipped (level 0 read in place), for reference

interleaved in one process, then the per-kernel times of each (orbx_profile_read, a pass of its own: event records on the
launch stream are not free).

    python tools/upstream_rate.py [--batch B] [--steps S] [--reps R]
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from orb_slam2_detailed_comments_amd import ORBextractor, synth, _capi

W, H = 640, 480


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


B, STEPS, REPS = arg("--batch", 1024), arg("--steps", 10), arg("--reps", 5)


def frames(n):
    """16 distinct scenes, rolled so that no two frames of a batch are the same bytes"""
    g = synth.stream(W, H, 16, stream_id=900)
    return np.stack([g[i % 16] if i < 16 else np.roll(g[i % 16], (5 * i % H, 11 * i % W), axis=(0, 1)) for i in range(n)])


def main():
    import torch
    dev = torch.device("cuda:0")
    d_img = torch.from_numpy(frames(B)).to(dev)
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device=dev)
    variants = []
    for name, mode, env in (("upstream", _capi.PYRAMID_UPSTREAM, None), ("fork-eager", _capi.PYRAMID_FORK_PADDED, "0"),
                            ("fork", _capi.PYRAMID_FORK_PADDED, None)):
        if env is not None:
            os.environ["ORBX_LEVEL0_INPLACE"] = env      # read when the handle is configured (its first extraction below)
        ex = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=B, device=0, pyramid_mode=mode)
        cap = ex.max_keypoints(W, H)
        bufs = (z(B, cap * 28), z(B, cap * 32), z(B, dt=torch.int32), z(B, dt=torch.int32))
        torch.cuda.synchronize()
        fn = (lambda ex=ex, bufs=bufs, cap=cap: ex.extract_batch_device(d_img, B, W, H, W, W * H, *bufs, cap))
        fn(); ex.synchronize()
        os.environ.pop("ORBX_LEVEL0_INPLACE", None)
        assert not bufs[3].any().item(), "extraction reported a non-zero status"
        # the batch takes the sub-batch pipeline; its first 16 frames must equal a 16-frame call (the serial sequence)
        small = (z(16, cap * 28), z(16, cap * 32), z(16, dt=torch.int32), z(16, dt=torch.int32))
        torch.cuda.synchronize()
        ex.extract_batch_device(d_img, 16, W, H, W, W * H, *small, cap); ex.synchronize()
        assert all(torch.equal(a[:16], b) for a, b in zip(bufs[:3], small[:3])), name + ": the batch differs from a 16-frame call"
        fn(); ex.synchronize()
        variants.append((name, ex, fn, bufs))

    def block(ex, fn):
        ex.synchronize()
        t = time.perf_counter()
        for _ in range(STEPS):
            fn()
        ex.synchronize()
        return (time.perf_counter() - t) / STEPS * 1e3

    for _, ex, fn, _ in variants * 2:
        block(ex, fn)
    times = {name: [] for name, _, _, _ in variants}
    for _ in range(REPS):
        for name, ex, fn, _ in variants:
            times[name].append(block(ex, fn))
    print(f"device-resident step, {B} frames (grey 640x480, 1000 features; {STEPS} steps per block, {REPS} interleaved blocks):")
    for name, _, _, bufs in variants:
        t = times[name]
        m = float(np.median(t))
        print(f"  {name:11s} {m:8.3f} ms  [{min(t):.3f} .. {max(t):.3f}]  {B / m * 1e3:8.0f} frames/s   {int(bufs[2].sum().item())} keypoints")
    print("per-kernel ms per step (HIP events on the launch stream; launches per step):")
    prof = {}
    for name, ex, fn, _ in variants:
        ex.profile_enable(0xffffffff)
        block(ex, fn)
        prof[name] = ex.profile_read()
        ex.profile_enable(0)
    names = [k for k in _capi.K_NAMES if any(prof[v][k][1] for v in prof)]
    print("  %-16s" % "kernel" + "".join("%22s" % v for v in prof))
    for k in names:
        print("  %-16s" % k + "".join("%15.3f (%3d)" % (prof[v][k][0] / STEPS, prof[v][k][1] // STEPS) for v in prof))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
