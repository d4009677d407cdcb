"""Microseconds per point of the batched MapPoint refresh against the same loop on the host.

    python tools/mappoint_rate.py [--out profiles/mappoint_batch.md]

Device: orbx_distinctive_descriptors_batch (rows copied from the host), orbx_distinctive_descriptors_batch_device (rows named in
a device pool that holds every keyframe's descriptors) and orbx_update_normal_and_depth_batch, one call for P = 1, 64, 1024,
8192 points, the caller's arrays already gathered.  Host, in the same run on the same box: the loop of single
MapPoint::ComputeDistinctiveDescriptors() / MapPoint::UpdateNormalAndDepth() calls over the same points, the bodies of
tests/compat_mappoint/map_model.cpp compiled -O3 (they copy the observation map and walk it, as the reference's do).  Two
observation-count mixes: "young map", N uniform in 2..8; "mature map", most points 5-30 observations and about one in a hundred
100-300.  The median of the repetitions is reported; results are checked against each other before anything is timed."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mappoint_harness as mh  # noqa: E402
import mappoint_model as mm  # noqa: E402
from orb_slam2_detailed_comments_amd import ORBextractor, _capi  # noqa: E402

NKF, NSLOTS = 300, 512
SIZES = (1, 64, 1024, 8192)


def build_host(out):
    cmd = [c for c in mh.build_cmd(out) if c != "-O1"] + ["-O3"]
    subprocess.check_call(cmd)
    return mh.Map(out)


def median_us(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(1)
    M = build_host(os.path.join(tempfile.mkdtemp(), "mappoint_host.so"))
    ex = ORBextractor(1000, 1.2, 8, 20, 7)
    L, h, P_ = _capi.lib(), ex.handle, _capi.ptr
    protos = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    kf_desc = protos[rng.integers(0, 8, (NKF, NSLOTS))]
    flips = rng.integers(0, 256, (NKF, NSLOTS, 3))
    ii, jj = np.indices((NKF, NSLOTS))
    for k in range(3):                                               # three flipped bits per row (some coincide)
        kf_desc[ii, jj, flips[..., k] >> 3] ^= (1 << (flips[..., k] & 7)).astype(np.uint8)
    kf_Ow = rng.normal(0, 3.0, (NKF, 3)).astype(np.float32)
    kf_oct = rng.integers(0, 8, (NKF, NSLOTS)).astype(np.int32)
    d_pool = torch.from_numpy(kf_desc.reshape(-1, 32)).cuda()
    lines = ["| mix | P | rows | descriptors, host rows | descriptors, device pool | host loop | normal / depth | host loop |",
             "|---|---|---|---|---|---|---|---|"]
    for mix, draw in (("young map", mm.young_mix), ("mature map", mm.mature_mix)):
        for npts in SIZES:
            counts = draw(rng, npts)
            M.call("mpt_reset")
            for k in range(NKF):
                M.keyframe(kf_desc[k], kf_oct[k], kf_Ow[k])
            ob = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
            rows_kf = np.concatenate([np.sort(rng.permutation(NKF)[:n]) for n in counts])
            rows_slot = np.repeat(np.arange(npts) % NSLOTS, counts)
            pos = (rng.normal(0, 3.0, (npts, 3)) + [0, 0, 8.0]).astype(np.float32)
            ref = rows_kf[ob[:-1]]
            for p in range(npts):
                M.point(pos[p], int(ref[p]), protos[0], np.zeros(3, np.float32), 0.0, 0.0)
                for k in rows_kf[ob[p]:ob[p + 1]]:
                    M.call("mpt_observe", p, int(k), p % NSLOTS)
            order = np.concatenate([[k for k, _ in M.obs(p)] for p in range(npts)])   # the map's own order
            rows_kf = order.astype(np.int64)
            desc = np.ascontiguousarray(kf_desc[rows_kf, rows_slot])
            obs_row = np.ascontiguousarray(rows_kf * NSLOTS + rows_slot, np.int64)
            centers = np.ascontiguousarray(kf_Ow[rows_kf])
            refc = np.ascontiguousarray(kf_Ow[ref])
            level = np.ascontiguousarray(kf_oct[ref, np.arange(npts) % NSLOTS])
            idx, med, out = np.zeros(npts, np.int32), np.zeros(npts, np.int32), np.zeros((npts, 32), np.uint8)
            idx2, out2 = np.zeros(npts, np.int32), np.zeros((npts, 32), np.uint8)
            nrm, dmin, dmax = np.zeros((npts, 3), np.float32), np.zeros(npts, np.float32), np.zeros(npts, np.float32)
            f_host = lambda: _capi.check(L.orbx_distinctive_descriptors_batch(h, npts, P_(ob), P_(desc), P_(idx), P_(med), P_(out)))
            f_dev = lambda: _capi.check(L.orbx_distinctive_descriptors_batch_device(h, P_(d_pool), NKF * NSLOTS, npts, P_(ob), P_(obs_row),
                                                                                    P_(idx2), None, P_(out2)))
            f_nd = lambda: _capi.check(L.orbx_update_normal_and_depth_batch(h, npts, P_(ob), P_(pos), P_(centers), P_(refc), P_(level),
                                                                            P_(nrm), P_(dmin), P_(dmax)))
            lst = np.arange(npts, dtype=np.int32)
            c_desc = lambda: M.call("mpt_single_loop", lst, npts, 1, 0)
            c_nd = lambda: M.call("mpt_single_loop", lst, npts, 0, 1)
            f_host(); f_dev(); f_nd(); c_desc(); c_nd()
            hd, ho = M.states(npts)
            assert np.array_equal(out, hd) and np.array_equal(out2, hd), "device and host descriptors differ"
            got = np.concatenate([nrm, dmin[:, None], dmax[:, None]], axis=1)
            assert np.array_equal(got.view(np.uint32), ho.view(np.uint32)), "device and host normal / depth differ"
            reps = 200 if npts <= 64 else 30 if npts <= 1024 else 8
            t = [median_us(f, reps) / npts for f in (f_host, f_dev, c_desc, f_nd, c_nd)]
            lines.append("| %s | %d | %d | %.2f | %.2f | %.2f | %.2f | %.2f |" % (mix, npts, ob[-1], t[0], t[1], t[2], t[3], t[4]))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
