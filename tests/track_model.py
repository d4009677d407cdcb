"""numpy restatement of the two-phase scheme behind the batched tracking matchers (csrc/orbx_kernels.hip: k_track_project,
k_track_cand, k_track_select), for both policies, plus the seeded scenes the CPU and GPU tests share.

Phase 1 (order-free): per point the candidates of its window in Frame::GetFeaturesInArea's visiting order (oracle.grid_query),
filtered by the tests that do not depend on the selection state (the u_right gate), reduced to the smallest key
(distance, visiting position) -- the two smallest for the map-point policy.  Phase 2 (in point order): a point whose stored
candidates are not blocked at its turn keeps them; otherwise its window is walked again without the blocked features.  The model
also counts what the tests need to be non-vacuous: rescans, overrides of a 0-observation point, accept events in dropped bins.

Projection (frame policy) is restated for ORBX_FP_STRICT only: every product and sum rounds to float on its own.
"""
import numpy as np
import oracle

TH_HIGH, HISTO = 100, 30
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
F32 = np.float32


def scale_factors(nlevels=8):
    return oracle.OracleExtractor(1000, 1.2, nlevels).tables()["scale"][:nlevels].copy()


def hamming_matrix(a, b):
    """[len(a), len(b)] Hamming distances of 32-byte descriptors"""
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)), np.int32)
    return POP[np.bitwise_xor(a[:, None, :], b[None, :, :])].sum(-1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ scenes
BOUNDS = (0.0, 200.0, 0.0, 150.0)
CAMERA = (120.0, 118.0, 100.0, 75.0)
MB, MBF = 0.1, 40.0


def _protos(rng, n, nproto=4, nflip=3):
    """descriptors near a few prototypes: small distances, many exact ties"""
    base = rng.integers(0, 256, (nproto, 32), dtype=np.uint8)
    d = base[rng.integers(0, nproto, n)].copy()
    for row in d:
        for b in rng.integers(0, 256, rng.integers(0, nflip + 1)):
            row[b >> 3] ^= np.uint8(1 << (b & 7))
    return d, base


def make_frame(rng, n, stereo=0.5, nproto=4):
    """a current frame: undistorted keypoints inside BOUNDS, descriptors, depths and u_right (-1 = monocular feature)"""
    k = np.zeros(n, oracle.KP_DTYPE)
    k["x"] = rng.uniform(BOUNDS[0] + 1, BOUNDS[1] - 1, n).astype(F32)
    k["y"] = rng.uniform(BOUNDS[2] + 1, BOUNDS[3] - 1, n).astype(F32)
    k["angle"] = rng.uniform(0, 360, n).astype(F32)
    k["octave"] = rng.choice(8, n, p=[.3, .2, .15, .1, .1, .05, .05, .05])
    d, base = _protos(rng, n, nproto)
    z = rng.uniform(1.0, 10.0, n)
    ur = np.where(rng.uniform(size=n) < stereo, k["x"] - MBF / z, -1.0).astype(F32)
    return dict(keys=k, desc=d, u_right=ur, depth=z, protos=base)


def _pose(rng, small=True):
    a = rng.normal(0, 0.02 if small else 0.2, 3)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + Kx + Kx @ Kx / 2
    u, _, vt = np.linalg.svd(R)
    T = np.eye(4)
    T[:3, :3] = u @ vt
    T[:3, 3] = rng.normal(0, 0.3, 3)
    return T


def make_ff_problem(rng, frame, nl, motion="side", th=15.0, mono=0, p_mp=0.85, scale=None):
    """last-frame points that project near features of `frame` (with duplicates, so that features are contended)"""
    scale = scale_factors() if scale is None else scale
    fx, fy, cx, cy = CAMERA
    kc, n = frame["keys"], len(frame["keys"])
    Tcw = _pose(rng)
    Rcw, tcw = Tcw[:3, :3], Tcw[:3, 3]
    twc = -Rcw.T @ tcw
    dz = {"forward": 0.5, "backward": -0.5, "side": 0.0}[motion]
    Tlw = np.eye(4)
    Tlw[:3, 3] = -twc + np.array([0.3, 0.0, dz])          # tlc = Rlw * twc + tlw = (0.3, 0, dz)
    kl = np.zeros(nl, oracle.KP_DTYPE)
    xw = np.zeros((nl, 3), F32)
    if n > 0:
        src = rng.integers(0, n, nl)
        u = kc["x"][src] + rng.normal(0, 1.5, nl)
        v = kc["y"][src] + rng.normal(0, 1.5, nl)
        z = frame["depth"][src] * (1 + rng.normal(0, 0.01, nl))
        kl["octave"] = np.clip(kc["octave"][src] + rng.integers(-1, 2, nl), 0, 7)
        kl["angle"] = np.mod(kc["angle"][src] + 20.0 + np.where(rng.uniform(size=nl) < 0.2, rng.uniform(0, 360, nl),
                                                                 rng.normal(0, 3, nl)), 360.0).astype(F32)
        mpd = frame["desc"][src].copy()
    else:
        u, v, z = rng.uniform(0, 200, nl), rng.uniform(0, 150, nl), rng.uniform(1, 10, nl)
        mpd = rng.integers(0, 256, (nl, 32), dtype=np.uint8)
    far = rng.uniform(size=nl) < 0.05                       # some projections outside the bounds, some behind the camera
    u = np.where(far, u + 500.0, u)
    z = np.where(rng.uniform(size=nl) < 0.05, -z, z)
    Xc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    xw[:] = ((Xc - tcw) @ Rcw).astype(F32)                  # Rcw^T (Xc - tcw)
    for row in mpd:
        for b in rng.integers(0, 256, rng.integers(0, 3)):
            row[b >> 3] ^= np.uint8(1 << (b & 7))
    return dict(th=F32(th), mono=int(mono), Tcw=Tcw.astype(F32), Tlw=Tlw.astype(F32), keys_un=kl,
                has_map_point=(rng.uniform(size=nl) < p_mp).astype(np.uint8), world_pos=xw, mp_desc=mpd,
                observations=rng.choice([0, 0, 1, 3], nl).astype(np.int32))


def make_mp_problem(rng, frame, nmp, th=3.0, p_view=0.85, occupied=0.2, cap=None):
    """local-map points projected near features of `frame`; `occupied` of the features already carry an observed MapPoint"""
    kf, n = frame["keys"], len(frame["keys"])
    proj = np.zeros((nmp, 3), F32)
    level = np.zeros(nmp, np.int32)
    if n > 0:
        src = rng.integers(0, n, nmp)
        proj[:, 0] = kf["x"][src] + rng.normal(0, 1.0, nmp)
        proj[:, 1] = kf["y"][src] + rng.normal(0, 1.0, nmp)
        proj[:, 2] = np.where(frame["u_right"][src] > 0, frame["u_right"][src], proj[:, 0] - 5) + rng.normal(0, 2.0, nmp)
        level[:] = np.clip(kf["octave"][src] + rng.integers(0, 2, nmp), 0, 7)
        mpd = frame["desc"][src].copy()
    else:
        proj[:] = rng.uniform(0, 150, (nmp, 3))
        mpd = rng.integers(0, 256, (nmp, 32), dtype=np.uint8)
    for row in mpd:
        for b in rng.integers(0, 256, rng.integers(0, 3)):
            row[b >> 3] ^= np.uint8(1 << (b & 7))
    fo = np.where(rng.uniform(size=max(n, cap or 0)) < occupied, rng.integers(1, 5, max(n, cap or 0)),
                  rng.choice([-1, 0], max(n, cap or 0))).astype(np.int32)
    return dict(th=F32(th), frame_observations=fo, in_view=(rng.uniform(size=nmp) < p_view).astype(np.uint8), proj=proj,
                level=level, view_cos=rng.choice([0.99, 0.9985, 0.9999], nmp).astype(F32), mp_desc=mpd,
                observations=rng.choice([0, 1, 2], nmp).astype(np.int32))


# ------------------------------------------------------------------------------------------------ the oracle on a scene
def oracle_ff(frame, p, check_ori=True, fp_mode=oracle.FP_STRICT, scale=None):
    scale = scale_factors() if scale is None else scale
    return oracle.search_by_projection_ff(frame["keys"], frame["desc"], frame["u_right"], p["Tcw"], CAMERA, BOUNDS, MB, MBF, scale,
                                          p["keys_un"], p["has_map_point"], p["world_pos"], p["mp_desc"], p["observations"],
                                          p["Tlw"], float(p["th"]), p["mono"], check_ori, fp_mode)


def oracle_mp(frame, p, nnratio, scale=None):
    scale = scale_factors() if scale is None else scale
    n = len(frame["keys"])
    return oracle.search_by_projection_mp(frame["keys"], frame["desc"], frame["u_right"], p["frame_observations"][:n], BOUNDS,
                                          scale, p["in_view"], p["proj"], p["level"], p["view_cos"], p["mp_desc"],
                                          p["observations"], float(p["th"]), float(nnratio))


# ------------------------------------------------------------------------------------------------ the model
def _gemm3(a, b, c):
    t = F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))
    return F32(np.float64(t) + np.float64(c))


def project_ff(p, scale):
    """per point (u, v, ur, r, min_level, max_level) or None: src/ORBmatcher.cc:1722-1783 with separate roundings (STRICT)"""
    fx, fy, cx, cy = (F32(v) for v in CAMERA)
    minx, maxx, miny, maxy = (F32(v) for v in BOUNDS)
    T, Tl = p["Tcw"].astype(F32), p["Tlw"].astype(F32)
    Rcw, tcw, Rlw, tlw = T[:3, :3], T[:3, 3], Tl[:3, :3], Tl[:3, 3]
    twc = [F32(-np.float64(F32(F32(F32(Rcw[0, r] * tcw[0]) + F32(Rcw[1, r] * tcw[1])) + F32(Rcw[2, r] * tcw[2])))) for r in range(3)]
    tlc2 = _gemm3(Rlw[2], twc, tlw[2])
    fwd, bwd = tlc2 > F32(MB) and not p["mono"], -tlc2 > F32(MB) and not p["mono"]
    out = []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(len(p["keys_un"])):
            if not p["has_map_point"][i]:
                out.append(None); continue
            pc = [_gemm3(Rcw[r], p["world_pos"][i], tcw[r]) for r in range(3)]
            invz = F32(np.float64(1.0) / np.float64(pc[2]))
            if invz < 0:
                out.append(None); continue
            u = F32(F32(F32(fx * pc[0]) * invz) + cx)
            v = F32(F32(F32(fy * pc[1]) * invz) + cy)
            if u < minx or u > maxx or v < miny or v > maxy:
                out.append(None); continue
            o = int(p["keys_un"]["octave"][i])
            lv = (o, -1) if fwd else (0, o) if bwd else (o - 1, o + 1)
            out.append((u, v, F32(u - F32(F32(MBF) * invz)), F32(p["th"] * scale[o]), lv[0], lv[1]))
    return out


def _window(frame, x, y, r, lo, hi):
    return oracle.grid_query(frame["keys"], BOUNDS, float(x), float(y), float(r), int(lo), int(hi))


def _best(cands, dist_row, ur_pt, r, u_right, blocked, two):
    """smallest (distance, position) keys over the candidates that pass the u_right gate and are not blocked"""
    keys = []
    for pos, j in enumerate(cands):
        if blocked is not None and blocked[j]:
            continue
        if u_right[j] > 0 and abs(F32(ur_pt - u_right[j])) > r:
            continue
        keys.append((int(dist_row[j]), pos, int(j)))
    keys.sort()
    return keys[:2] if two else keys[:1]


def model_ff(frame, p, check_ori=True, scale=None):
    """returns (nmatches, matched_last[n], stats)"""
    scale = scale_factors() if scale is None else scale
    kc, n = frame["keys"], len(frame["keys"])
    matched = np.full(n, -1, np.int32)
    stats = dict(rescans=0, overrides=0, dropped_events=0, kept_overridden=0, live=0)
    if n == 0:
        return 0, matched, stats
    q = project_ff(p, scale)
    D = hamming_matrix(p["mp_desc"], frame["desc"])
    stored = [None if qi is None else (_window(frame, *qi[:2], qi[3], qi[4], qi[5])) for qi in q]
    first = [None if c is None else _best(c, D[i], q[i][2], q[i][3], frame["u_right"], None, False) for i, c in enumerate(stored)]
    blocked = np.zeros(n, bool)
    events = []
    for i, b in enumerate(first):
        if not b or b[0][0] > TH_HIGH:
            continue
        stats["live"] += 1
        if blocked[b[0][2]]:
            stats["rescans"] += 1
            b = _best(stored[i], D[i], q[i][2], q[i][3], frame["u_right"], blocked, False)
            if not b or b[0][0] > TH_HIGH:
                continue
        j = b[0][2]
        if matched[j] >= 0:
            stats["overrides"] += 1
        matched[j] = i
        blocked[j] = p["observations"][i] > 0
        events.append((i, j))
    nm = len(events)
    if check_ori:
        bins = []
        for i, j in events:
            rot = F32(p["keys_un"]["angle"][i] - kc["angle"][j])
            if rot < 0:
                rot = F32(rot + F32(360.0))
            b = int(np.floor(np.float64(F32(rot * F32(HISTO / F32(360.0)))) + 0.5))     # roundf of a non-negative float
            bins.append(0 if b == HISTO else b)
        hist = np.bincount(bins, minlength=HISTO) if bins else np.zeros(HISTO, int)
        keep = set(oracle.three_maxima(hist))
        final = {}
        for (i, j), b in zip(events, bins):
            final[j] = i
        for (i, j), b in zip(events, bins):
            if b not in keep:
                matched[j] = -1
                nm -= 1
                stats["dropped_events"] += 1
                if final[j] != i:
                    stats["kept_overridden"] += 1           # a dropped event whose feature a later event had taken over
    return nm, matched, stats


def model_mp(frame, p, nnratio, scale=None):
    """returns (nmatches, assigned[n], stats)"""
    scale = scale_factors() if scale is None else scale
    n = len(frame["keys"])
    assigned = np.full(n, -1, np.int32)
    stats = dict(rescans=0, live=0, ratio_rejects=0)
    if n == 0:
        return 0, assigned, stats
    D = hamming_matrix(p["mp_desc"], frame["desc"])
    octv = frame["keys"]["octave"]
    blocked = p["frame_observations"][:n] > 0
    nm = 0
    bfactor = float(p["th"]) != 1.0
    for i in range(len(p["in_view"])):
        if not p["in_view"][i]:
            continue
        lvl = int(p["level"][i])
        r = F32(2.5) if p["view_cos"][i] > 0.998 else F32(4.0)
        if bfactor:
            r = F32(r * p["th"])
        r = F32(r * scale[lvl])
        cands = _window(frame, p["proj"][i, 0], p["proj"][i, 1], r, lvl - 1, lvl)
        b = _best(cands, D[i], p["proj"][i, 2], r, frame["u_right"], None, True)
        if not b or b[0][0] > TH_HIGH:
            continue
        stats["live"] += 1
        if any(blocked[k[2]] for k in b):
            stats["rescans"] += 1
            b = _best(cands, D[i], p["proj"][i, 2], r, frame["u_right"], blocked, True)
            if not b or b[0][0] > TH_HIGH:
                continue
        d1, l1 = b[0][0], int(octv[b[0][2]])
        d2, l2 = (b[1][0], int(octv[b[1][2]])) if len(b) > 1 else (256, -1)
        if l1 == l2 and F32(d1) > F32(F32(nnratio) * F32(d2)):
            stats["ratio_rejects"] += 1
            continue
        j = b[0][2]
        assigned[j] = i
        blocked[j] = p["observations"][i] > 0
        nm += 1
    return nm, assigned, stats
