"""Seeded scenes for Optimizer::OptimizeSim3 (orbx_optimize_sim3_batch): two cameras with K1 != K2, a true Sim3 S12 (x1 = s R x2
+ t), a start perturbed by a few degrees, a few centimetres and a few percent of scale, points in front of both cameras,
observation noise in pixels and planted outliers.  A scene is the dict optimizer.optimize_sim3_batch takes, plus the truth."""
import numpy as np

CAMERA1 = np.array([517.3, 516.5, 318.6, 255.3], np.float32)
CAMERA2 = np.array([535.4, 539.2, 320.1, 247.6], np.float32)
INV_SIGMA2 = (1.0 / np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
TH2 = np.float32(10.0)                     # LoopClosing::ComputeSim3: OptimizeSim3(..., 10, mbFixScale)
PREFILL_KEEP = 0xA5


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def make(seed, n, fix_scale=False, noise=0.0, outlier_frac=0.0, rot_deg=3.0, trans=0.05, scale_pct=3.0, gross=(15.0, 60.0)):
    rng = np.random.default_rng(seed)
    s_true = 1.0 if fix_scale else float(rng.uniform(0.8, 1.25))
    R_true = rodrigues(rng.normal(size=3) * np.deg2rad(8.0))
    t_true = rng.uniform(-0.4, 0.4, 3)
    x1 = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.5, 8.0, n)], 1)
    x2 = ((x1 - t_true) @ R_true) / s_true                  # S12^-1 x1
    x1f, x2f = x1.astype(np.float32), x2.astype(np.float32)

    def proj(K, x):
        return np.stack([x[:, 0] / x[:, 2] * K[0] + K[2], x[:, 1] / x[:, 2] * K[1] + K[3]], 1)
    obs1 = proj(CAMERA1.astype(np.float64), x1) + rng.normal(size=(n, 2)) * noise
    obs2 = proj(CAMERA2.astype(np.float64), x2) + rng.normal(size=(n, 2)) * noise
    planted = rng.uniform(size=n) < outlier_frac
    off = rng.uniform(gross[0], gross[1], n)[:, None] * np.stack([np.cos(a := rng.uniform(0, 2 * np.pi, n)), np.sin(a)], 1)
    which = rng.uniform(size=n) < 0.5
    obs1 = np.where((planted & which)[:, None], obs1 + off, obs1)
    obs2 = np.where((planted & ~which)[:, None], obs2 + off, obs2)
    l1, l2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    R0 = rodrigues(rng.normal(size=3) * np.deg2rad(rot_deg) / np.sqrt(3)) @ R_true
    t0 = t_true + rng.normal(size=3) * trans / np.sqrt(3)
    s0 = s_true if fix_scale else s_true * (1 + rng.uniform(-1, 1) * scale_pct / 100)
    return dict(n=n, x1c=x1f, x2c=x2f, obs1=obs1.astype(np.float32), obs2=obs2.astype(np.float32),
                inv_sigma2_1=INV_SIGMA2[l1].copy(), inv_sigma2_2=INV_SIGMA2[l2].copy(), camera1=CAMERA1, camera2=CAMERA2,
                R=R0.astype(np.float32), t=t0.astype(np.float32), s=np.float32(s0), th2=TH2, fix_scale=int(fix_scale),
                R_true=R_true, t_true=t_true, s_true=s_true, planted=planted)


def variant(scene, **kw):
    out = dict(scene)
    out.update(kw)
    return out


def problem(s, keep=None):
    """what optimize_sim3_batch reads, with a prefilled keep row of n + 3 bytes"""
    p = {k: s[k] for k in ("x1c", "x2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "camera1", "camera2", "R", "t", "s", "th2",
                           "fix_scale")}
    p["keep"] = np.full(s["n"] + 3, PREFILL_KEEP, np.uint8) if keep is None else keep
    return p
