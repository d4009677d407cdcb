"""Planted inputs of the front-end suites (tests/test_frontend_cpu.py, tests/test_frontend_gpu.py): rectification maps, colour
frames and distortion models whose edge classes are put there on purpose.  Every scene returns its inputs and a dict of class
masks computed from the MODEL's view of the inputs (tests/frontend_model.py); test_frontend_cpu.py asserts that each class a
scene claims is non-empty, so a scene cannot silently stop planting what the GPU tests rely on."""
import numpy as np
import frontend_model as M

# W, H -> padded width pw = W + 38: 135 leaves the 4-pixel store tail of k_pyr_l0_remap / k_pyr_l0_color partly empty, 104
# fills it, 268 needs two block columns (256 padded pixels each)
GEOMETRIES = [(97, 75), (66, 50), (230, 60)]

NONFINITE = [np.nan, np.inf, -np.inf, 2.0 ** 26, -2.0 ** 26, 2.0 ** 27, -2.0 ** 27, 7e7, -7e7, 1e9]

EDGE_CLASSES = ["left", "right", "top", "bottom", "corner_tl", "corner_tr", "corner_bl", "corner_br",
                "out_left", "out_right", "out_top", "out_bottom", "short_hi_x", "short_lo_x", "short_hi_y", "short_lo_y",
                "neg_frac_x", "neg_frac_y", "tie_pos", "tie_neg", "tie_carry", "bad_x", "bad_y", "bad_xy"]


def raw_frames(w, h, n, seed):
    """uniform random bytes with planted runs of 0 and 255; row 0 and column 0 never hold a 0, so that a map entry wrongly
    digested to column / row 0 reads something the border value 0 differs from"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    for i in range(n):
        for k in range(6):
            y, x, run = int(rng.integers(1, h)), int(rng.integers(1, w - 12)), int(rng.integers(3, 12))
            f[i, y, x:x + run] = 0 if k % 2 else 255
    f[:, 0, :] = np.maximum(f[:, 0, :], 1 + (f[:, 0, :] >> 1))
    f[:, :, 0] = np.maximum(f[:, :, 0], 1 + (f[:, :, 0] >> 1))
    return f


def _classes(mx, my, w, h):
    d = M.digest_full(mx, my)
    ix, iy, fx, fy, bx, by = d["ix"], d["iy"], d["fx"], d["fy"], d["bad_x"], d["bad_y"]
    xin, yin = (ix >= 0) & (ix < w - 1), (iy >= 0) & (iy < h - 1)      # both taps of that axis inside
    fr = (fx != 0) & (fy != 0)
    with np.errstate(invalid="ignore", over="ignore"):
        px, py = mx * np.float32(32), my * np.float32(32)
        tie_x = np.isfinite(px) & (np.abs(px) < 2.0 ** 20) & (px - np.floor(px) == 0.5)
        tie_y = np.isfinite(py) & (np.abs(py) < 2.0 ** 20) & (py - np.floor(py) == 0.5)
        carry = (tie_x & (mx > 0) & (ix == np.floor(mx) + 1) & (fx == 0)) | (tie_y & (my > 0) & (iy == np.floor(my) + 1) & (fy == 0))
    return {
        "left": (ix == -1) & (fx != 0) & yin, "right": (ix == w - 1) & (fx != 0) & yin,
        "top": (iy == -1) & (fy != 0) & xin, "bottom": (iy == h - 1) & (fy != 0) & xin,
        "corner_tl": (ix == -1) & (iy == -1) & fr, "corner_tr": (ix == w - 1) & (iy == -1) & fr,
        "corner_bl": (ix == -1) & (iy == h - 1) & fr, "corner_br": (ix == w - 1) & (iy == h - 1) & fr,
        "out_left": (ix == -2) & yin, "out_right": (ix == w) & yin, "out_top": (iy == -2) & xin, "out_bottom": (iy == h) & xin,
        "short_hi_x": (ix == 32767) & ~bx & (fx != 0), "short_lo_x": (ix == -32768) & ~bx & (fx != 0),
        "short_hi_y": (iy == 32767) & ~by & (fy != 0), "short_lo_y": (iy == -32768) & ~by & (fy != 0),
        "neg_frac_x": (ix == -1) & (fx == 24), "neg_frac_y": (iy == -1) & (fy == 24),
        "tie_pos": (tie_x & (mx > 0)) | (tie_y & (my > 0)), "tie_neg": (tie_x & (mx < 0)) | (tie_y & (my < 0)), "tie_carry": carry,
        "bad_x": bx & ~by & (iy >= 0) & (iy < h), "bad_y": by & ~bx & (ix >= 0) & (ix < w), "bad_xy": bx & by,
        "inside": xin & yin, "identity": (ix == np.arange(w)[None, :]) & (iy == np.arange(h)[:, None]) & (fx == 0) & (fy == 0),
    }


def edge_maps(w, h, seed=0):
    """a gentle base map (x + 0.37, y + 0.71) with every edge class planted, spread evenly over the image so that the planted
    entries fall into every block and next to ordinary ones.  Returns mx, my, classes, planted (the tie and non-finite counts)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    mx = (xx + 0.37).astype(np.float32); my = (yy + 0.71).astype(np.float32)
    vx = lambda: np.float32(int(rng.integers(1, w - 2)) + 0.3125)     # a valid coordinate with a fraction (10/32)
    vy = lambda: np.float32(int(rng.integers(1, h - 2)) + 0.5625)
    ent = []
    for xv in (-0.6, w - 1 + 0.4):                                    # one tap column outside / three taps outside
        ent.append((xv, vy()))
        for yv in (-0.6, h - 1 + 0.4):
            ent.append((xv, yv))
    for yv in (-0.6, h - 1 + 0.4):
        ent.append((vx(), yv))
    ent += [(-2 + 0.4, vy()), (w + 0.4, vy()), (vx(), -2 + 0.4), (vx(), h + 0.4)]           # all taps outside by one
    ent += [(40000.3, vy()), (-40000.3, vy()), (vx(), 40000.3), (vx(), -40000.3)]           # beyond the short range
    ent += [(-0.25, vy()), (vx(), -0.25)]                                                   # ix = -1, fx = 24
    ties = []
    for j in range(32):                                                                     # exact in float32: n < 2^8, 1/64 steps
        n = int(rng.integers(1, min(w, h) - 2))
        ties += [n + (2 * j + 1) / 64.0, -(2 * j + 1) / 64.0]
    for t in ties:
        assert float(np.float32(t)) == t
        ent += [(t, vy()), (vx(), t)]
    for v in NONFINITE:                                                                     # in map_x alone, map_y alone, both
        ent += [(v, np.float32(int(rng.integers(1, h - 2)))), (np.float32(int(rng.integers(1, w - 2))), v), (v, v)]
        ent += [(v, vy()), (vx(), v)]
    step = (w * h) // len(ent)
    assert step >= 2
    pos = np.arange(len(ent)) * step + step // 2
    with np.errstate(over="ignore"):
        mx.reshape(-1)[pos] = np.array([e[0] for e in ent], np.float64).astype(np.float32)
        my.reshape(-1)[pos] = np.array([e[1] for e in ent], np.float64).astype(np.float32)
    return mx, my, _classes(mx, my, w, h), dict(ties=len(ties), nonfinite=len(NONFINITE))


def scrambled_maps(w, h, seed=1):
    """independent uniform coordinates in [-3, w + 3] x [-3, h + 3]: neighbouring lanes read far apart"""
    rng = np.random.default_rng(seed)
    mx = rng.uniform(-3, w + 3, (h, w)).astype(np.float32); my = rng.uniform(-3, h + 3, (h, w)).astype(np.float32)
    c = _classes(mx, my, w, h)
    c["outside"] = ~c["inside"]
    return mx, my, c


def identity_maps(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    mx, my = xx.astype(np.float32), yy.astype(np.float32)
    return mx, my, _classes(mx, my, w, h)


def map_scenes(w, h):
    """name -> (mx, my, classes, claimed class names)"""
    ex, ey, ec, _ = edge_maps(w, h)
    sx, sy, sc = scrambled_maps(w, h)
    jx, jy, jc = identity_maps(w, h)
    return {"edges": (ex, ey, ec, EDGE_CLASSES), "scrambled": (sx, sy, sc, ["inside", "outside", "left", "right", "top", "bottom"]),
            "identity": (jx, jy, jc, ["identity"])}


# ---------------------------------------------------------------------------------------------------------- colour frames
COLOUR_CLASSES = ["pure_r", "pure_g", "pure_b", "black", "white", "noise"]


def colour_frames(w, h, nch, n, seed=0, rgb=True):
    """[n, h, w, nch] frames of 8 x 8 tiles cycling through pure R, pure G, pure B (255 in one channel), black, white and random
    colour noise, the cycle shifted per frame; a fourth channel holds random bytes.  `rgb` says where R sits (channel 0) --
    the SAME scene in BGR order has R in channel 2.  Returns frames and per-frame class masks [n, h, w]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.zeros((n, h, w, nch), np.uint8)
    masks = {c: np.zeros((n, h, w), bool) for c in COLOUR_CLASSES}
    r, b = (0, 2) if rgb else (2, 0)
    for i in range(n):
        t = (xx // 8 + yy // 8 + i) % 6
        noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for cid, name in enumerate(COLOUR_CLASSES):
            m = t == cid
            masks[name][i] = m
            if name == "pure_r": f[i, m, r] = 255
            elif name == "pure_g": f[i, m, 1] = 255
            elif name == "pure_b": f[i, m, b] = 255
            elif name == "white": f[i, m, :3] = 255
            elif name == "noise": f[i, m, :3] = noise[m]
        if nch == 4:
            f[i, :, :, 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return f, masks


# ---------------------------------------------------------------------------------------------------------- distortion models
TUM1_K = (517.306408, 516.469215, 318.643040, 255.313989)                       # Examples/Monocular/TUM1.yaml
TUM1_D = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
# 8 terms (rational: k4, k5, k6) and 12 terms (thin prism: s1..s4), mild enough that the forward model stays monotone over
# 640 x 480 and 50 pixels beyond (checked by test_frontend_cpu.py::test_forward_models_are_monotone)
D8 = (0.12, -0.21, 0.0007, -0.0004, 0.05, 0.03, -0.02, 0.01)
D12 = D8 + (0.0011, -0.0006, 0.0009, 0.0004)
DIST_MODELS = {"tum1_4": TUM1_D[:4], "tum1_5": TUM1_D, "rational_8": D8, "prism_12": D12, "prism_14_zero_tilt": D12 + (0.0, 0.0)}
IMAGE_WH = (640, 480)


def keypoints(n, dtype, seed=0, w=IMAGE_WH[0], h=IMAGE_WH[1]):
    """n keypoint records: the image corners, the principal point and points up to 50 pixels outside the image first (as many as
    fit), random interior points after them; the other fields hold values a copy must preserve"""
    rng = np.random.default_rng(seed)
    cx, cy = np.float32(TUM1_K[2]), np.float32(TUM1_K[3])
    fixed = [(0, 0), (w, 0), (0, h), (w, h), (cx, cy), (-50, -50), (w + 50, -50), (-50, h + 50), (w + 50, h + 50), (-37.5, h / 2),
             (w + 12.25, h / 3), (w / 2, -50), (w / 3, h + 44.75)]
    k = np.zeros(n, dtype)
    k["x"] = rng.uniform(0, w, n).astype(np.float32); k["y"] = rng.uniform(0, h, n).astype(np.float32)
    m = min(n, len(fixed))
    if n == 1:
        fixed = [fixed[8]]
    k["x"][:m] = [p[0] for p in fixed[:m]]; k["y"][:m] = [p[1] for p in fixed[:m]]
    k["size"] = 31; k["angle"] = rng.uniform(0, 360, n).astype(np.float32); k["response"] = rng.integers(7, 255, n)
    k["octave"] = rng.integers(0, 8, n); k["class_id"] = -1
    x, y = k["x"], k["y"]
    classes = {"corner": ((x == 0) | (x == w)) & ((y == 0) | (y == h)), "principal": (x == cx) & (y == cy),
               "outside": (x < 0) | (x > w) | (y < 0) | (y > h), "interior": (x > 0) & (x < w) & (y > 0) & (y < h)}
    return k, classes


COUNTS = [1, 255, 256, 257]   # around the 256-thread block of k_undistort / k_rgbd
