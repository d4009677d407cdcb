"""Synthetic LocalBundleAdjustment problems with known poses and points for tests/test_localba_cpu.py and
tests/test_localba_gpu.py: keyframes on a short arc looking at a cloud of points two to ten metres in front of them, the camera
and the pyramid of tests/pose_scenes.py."""
import numpy as np

from pose_scenes import CAMERA4, MBF, INV_SIGMA2, LEVEL_SIGMA, NLEVELS, pose


def make(seed, nlocal, nfixed, npoints, mode="mixed", noise=0.0, outlier_frac=0.0, perturb=(0.02, 0.01, 0.03), min_obs=2,
         max_obs=None, full_kf=None, local_fixed=(), second_round=True):
    """perturb = (metres, radians) on the local keyframes' start poses and metres on the start points; the fixed keyframes start
    at the truth.  Every point is seen by a random subset of min_obs..max_obs keyframes (default: all); full_kf = (k, n): keyframe
    k sees exactly the first n points.  Returns the problem dict of optimizer.local_bundle_adjustment_batch plus Tcw_true,
    world_true, planted (bool per observation: gross outlier) and gross (its offset in pixels)."""
    rng = np.random.default_rng(seed)
    nkf = nlocal + nfixed
    Ttrue = np.stack([pose(rng.normal(0, 0.03, 3) + [0, 0.04 * (i - nkf / 2), 0], rng.normal(0, 0.05, 3) + [0.25 * (i - nkf / 2), 0, 0])
                      for i in range(nkf)]).astype(np.float32) if nkf else np.zeros((0, 4, 4), np.float32)
    z = rng.uniform(2.0, 10.0, npoints)
    world = np.stack([rng.uniform(-0.6, 0.6, npoints) * z, rng.uniform(-0.45, 0.45, npoints) * z, z], 1).astype(np.float32)
    max_obs = nkf if max_obs is None else min(max_obs, nkf)
    begin, okf, obs, w, planted, gross = [0], [], [], [], [], []
    for p in range(npoints):
        k = int(rng.integers(min(min_obs, nkf), max_obs + 1)) if nkf else 0
        seen = set(rng.permutation(nkf)[:k].tolist())
        if full_kf is not None:
            seen.discard(full_kf[0])
            if p < full_kf[1]:
                seen.add(full_kf[0])
        seen = rng.permutation(sorted(seen))                  # the caller's order: no particular one
        for i in seen:
            T = Ttrue[i].astype(np.float64)
            pc = T[:3, :3] @ world[p].astype(np.float64) + T[:3, 3]
            u, v = CAMERA4[0] * pc[0] / pc[2] + CAMERA4[2], CAMERA4[1] * pc[1] / pc[2] + CAMERA4[3]
            ur = u - float(MBF) / pc[2]
            octave = int(rng.integers(0, NLEVELS))
            sg = LEVEL_SIGMA[octave]
            u, v, ur = u + rng.normal(0, noise) * sg, v + rng.normal(0, noise) * sg, ur + rng.normal(0, noise) * sg
            pl = rng.random() < outlier_frac
            g = rng.uniform(12, 40) * sg if pl else 0.0
            ang = rng.uniform(0, 2 * np.pi)
            u, v = u + g * np.cos(ang), v + g * np.sin(ang)
            stereo = {"mono": False, "stereo": True, "mixed": rng.random() < 0.5}[mode]
            okf.append(i); obs.append((u, v, ur if stereo else -1.0)); w.append(INV_SIGMA2[octave]); planted.append(pl); gross.append(g)
        begin.append(len(okf))
    T0 = Ttrue.copy()
    for i in range(nlocal):
        d = pose(rng.normal(0, 1, 3) * perturb[1] / np.sqrt(3), rng.normal(0, 1, 3) * perturb[0] / np.sqrt(3))
        T0[i] = (d @ Ttrue[i].astype(np.float64)).astype(np.float32)
    lf = np.zeros(nlocal, np.uint8)
    for i in local_fixed:
        lf[i] = 1
        T0[i] = Ttrue[i]
    world0 = (world + rng.normal(0, 1, world.shape) * perturb[2] / np.sqrt(3)).astype(np.float32)
    return dict(nlocal=nlocal, Tcw=T0.reshape(-1, 16), local_fixed=lf, camera=CAMERA4, bf=MBF, world=world0,
                obs_begin=np.array(begin, np.int32), obs_kf=np.array(okf, np.int32).reshape(-1),
                obs=np.array(obs, np.float32).reshape(-1, 3), inv_sigma2=np.array(w, np.float32).reshape(-1),
                second_round=second_round, Tcw_true=Ttrue.reshape(-1, 16), world_true=world,
                planted=np.array(planted, bool), gross=np.array(gross))


def keep_obs(p, keep):
    """the problem with only the observations where keep is set (CSR rebuilt); per-observation extras follow"""
    keep = np.asarray(keep, bool)
    q = dict(p)
    pt = np.repeat(np.arange(len(p["world"])), np.diff(p["obs_begin"]))
    q["obs_begin"] = np.concatenate([[0], np.cumsum(np.bincount(pt[keep], minlength=len(p["world"])))]).astype(np.int32)
    for k in ("obs_kf", "obs", "inv_sigma2", "planted", "gross"):
        q[k] = p[k][keep]
    return q
