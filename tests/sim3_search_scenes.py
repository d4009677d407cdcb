"""Scenes for orbx_search_by_sim3_batch: generators that return the C-ABI arrays (a dict keyframes / problems / camera4 / bounds4,
the arguments of ORBmatcher.SearchBySim3Batch) and play() that builds the same scene in a harness speaking the ABI of
tests/compat_runtime/harness.cpp (the shim harness, or the reference's compiled ORBmatcher.cc in oracle/_ref/).

Keyframes hold at most 300 features and a scene at most 6 problems.  A problem's already-matched features are `pairs`: (i1, i2)
with i2 a slot of kf2 that holds a point (vpMatches12[i1] = that point, so vbAlreadyMatched2[i2] is set as :1470-1483 do) or -1 (a
point kf2 does not observe).  The planted scenes run under identity poses and an identity Sim3, where a point's camera coordinates
in the other keyframe ARE its world position, so every threshold is hit exactly; each planted item is asserted on the model by
planted_checks(), so a generator that stops producing a case fails."""
import numpy as np

import sim3_search_model as sm
from compat_scenes import CX, CY, FX, H_, KP, PERMS, W, F32 as CF32, Scene, flips, i32, keys_near, pose
from test_ref_matcher import float_camera_point, rodrigues

F = np.float32
CAMERA4 = np.array([FX, FX, CX, CY], F)
BOUNDS4 = np.array([0, W, 0, H_], F)
TH = 7.5
NLEVELS, SCALE_FACTOR = 8, 1.2
EYE4 = np.eye(4, dtype=F)


def scale_table():
    sf = np.ones(NLEVELS, F)
    for l in range(1, NLEVELS):
        sf[l] = F(sf[l - 1] * F(SCALE_FACTOR))
    return sf


class KF:
    """a keyframe under construction"""

    def __init__(self, Tcw=EYE4):
        self.Tcw = np.array(Tcw, F)
        self.rows = []

    def feat(self, x, y, octave=0, desc=None, point=None, rng=None):
        """point: None or dict P (world position), dmin, dmax, desc"""
        d = np.zeros(32, np.uint8) if desc is None else np.asarray(desc, np.uint8)
        self.rows.append((F(x), F(y), int(octave), d, point))
        return len(self.rows) - 1

    def build(self):
        n = len(self.rows)
        keys = np.zeros(n, KP)
        desc, pdesc = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
        has, pos, dmin, dmax = np.zeros(n, np.uint8), np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F)
        for i, (x, y, o, d, pt) in enumerate(self.rows):
            keys[i]["x"], keys[i]["y"], keys[i]["octave"], keys[i]["angle"], keys[i]["size"], keys[i]["class_id"] = x, y, o, 10.0, 31.0, -1
            desc[i] = d
            if pt is not None:
                has[i], pos[i], dmin[i], dmax[i], pdesc[i] = 1, pt["P"], pt["dmin"], pt["dmax"], pt["desc"]
        return dict(keys_un=keys, desc=desc, Tcw=self.Tcw, has_point=has, world_pos=pos, min_distance=dmin, max_distance=dmax,
                    point_desc=pdesc)


def problem(kf1, kf2, n1, n2, s12=1.0, R12=None, t12=None, th=TH, pairs=()):
    m1, m2 = np.zeros(n1, np.uint8), np.zeros(n2, np.uint8)
    for a, b in pairs:
        m1[a] = 1
        if b >= 0: m2[b] = 1
    return dict(kf1=kf1, kf2=kf2, s12=float(F(s12)), R12=np.eye(3, dtype=F) if R12 is None else np.array(R12, F),
                t12=np.zeros(3, F) if t12 is None else np.array(t12, F), th=th, matched1=m1, matched2=m2, pairs=list(pairs))


def scene(kfs, problems):
    assert all(len(k["keys_un"]) <= 300 for k in kfs) and len(problems) <= 6
    return dict(keyframes=kfs, problems=problems, camera4=CAMERA4, bounds4=BOUNDS4)


def point_at(P, desc, level=0, dist=None, dmin=None, dmax=None):
    """a MapPoint whose PredictScale at distance `dist` gives `level` with half a level to spare"""
    P = np.asarray(P, F)
    dist = float(np.linalg.norm(P.astype(np.float64))) if dist is None else dist
    dmax = F(dist * SCALE_FACTOR ** (level - 0.5)) if dmax is None else F(dmax)
    dmin = F(dmax / F(SCALE_FACTOR ** 7)) if dmin is None else F(dmin)
    return dict(P=P, dmin=dmin, dmax=dmax, desc=np.asarray(desc, np.uint8))


def at_pixel(u, v, z=2.0):
    """world position (identity poses) that projects to (u, v): exact for u, v multiples of 1/8 and z a power of two"""
    return np.array([(u - CX) / FX * z, (v - CY) / FX * z, z], F)


def rnd_desc(rng, n=None):
    return rng.integers(0, 256, 32 if n is None else (n, 32), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ general scenes
def _pair_scene(rng, exact, nprob):
    """nprob problems sharing KF1: points with keypoints near both projections, as case_sim3 of tests/test_ref_matcher.py"""
    kfs, probs = [None], []
    if exact:
        R1, t1 = PERMS[1], np.array([0.5, 0.25, -0.125], F)
    else:
        R1, t1 = rodrigues(rng), rng.uniform(-0.5, 0.5, 3).astype(F)
    K1 = KF(pose(R1, t1))
    npts = 60
    all_pairs = []
    for k in range(nprob):
        if exact:
            R2, t2 = PERMS[(k + 2) % 3], np.array([-0.25, 0.5, 0.25], F) * (k + 1)
            s12, R12, t12 = 2.0 ** (k % 3 - 1), PERMS[(k + 1) % 2], np.zeros(3, F)      # (the identity or x <-> y: z stays the depth)
        else:
            R2, t2 = rodrigues(rng), rng.uniform(-0.5, 0.5, 3).astype(F)
            s12, R12, t12 = float(F(rng.uniform(0.7, 1.4))), rodrigues(rng, 0.15), rng.uniform(-0.05, 0.05, 3).astype(F)
        K2 = KF(pose(R2, t2))
        c2s = []
        while len(c2s) < npts:
            if exact:
                from compat_scenes import exact_camera_point
                c2, _ = exact_camera_point(rng)
            else:
                c2, _ = float_camera_point(rng)
            c1 = s12 * (np.asarray(R12, np.float64) @ c2) + t12
            if c1[2] > 0.3 and 20 < FX * c1[0] / c1[2] + CX < W - 20 and 20 < FX * c1[1] / c1[2] + CY < H_ - 20 and \
                    20 < FX * c2[0] / c2[2] + CX < W - 20 and 20 < FX * c2[1] / c2[2] + CY < H_ - 20:
                c2s.append((c2, c1))
        first1 = len(K1.rows)
        for j, (c2, c1) in enumerate(c2s):
            lv = int(rng.integers(0, 7))
            d = rnd_desc(rng)
            d1, d2 = float(np.linalg.norm(c1)), float(np.linalg.norm(c2))
            u1, v1 = FX * c1[0] / c1[2] + CX, FX * c1[1] / c1[2] + CY
            u2, v2 = FX * c2[0] / c2[2] + CX, FX * c2[1] / c2[2] + CY
            X1 = np.asarray(R1, np.float64).T @ (c1 - t1.astype(np.float64))      # kf1's point: where the Sim3 puts c2 from c1
            X2 = np.asarray(R2, np.float64).T @ (c2 - t2.astype(np.float64))
            nf = lambda: int(rng.choice([0, 6, 20, 50, 99, 100, 101, 120]))
            off = lambda: float(rng.integers(-8, 9)) / 4.0
            oc = lambda: int(np.clip(lv - rng.integers(-1, 3), 0, NLEVELS - 1))
            p1 = point_at(X1, d, lv, dist=d2) if rng.uniform() < 0.85 else None   # searched in kf2 at distance |c2|
            p2 = point_at(X2, d, lv, dist=d1) if rng.uniform() < 0.85 else None
            if j % 15 == 14 and p1 is not None: p1["dmax"] = F(d2 / 4)          # outside the distance band
            K1.feat(u1 + off(), v1 + off(), oc(), flips(rng, d, nf()), p1)
            K2.feat(u2 + off(), v2 + off(), oc(), flips(rng, d, nf()), p2)
        for _ in range(10):
            K2.feat(rng.uniform(10, W - 10), rng.uniform(10, H_ - 10), int(rng.integers(0, 8)), rnd_desc(rng))
        pairs = []
        for j in rng.choice(npts, 5, replace=False):
            i2 = int(j) if K2.rows[int(j)][4] is not None and rng.uniform() < 0.7 else -1
            pairs.append((first1 + int(j), i2))
        all_pairs.append((k + 1, s12, R12, t12, pairs))
        kfs.append(K2)
    built = [K1.build()] + [k.build() for k in kfs[1:]]
    n1 = len(built[0]["keys_un"])
    for k2, s12, R12, t12, pairs in all_pairs:
        probs.append(problem(0, k2, n1, len(built[k2]["keys_un"]), s12, R12, t12, pairs=pairs))
    return scene(built, probs)


def exact_scene(seed=0):
    return _pair_scene(np.random.default_rng(4100 + seed), True, 3)


def float_scene(thr, seed=0):
    """seeded rodrigues poses; every searched point's PredictScale ratio is at least 1e-5 (relative) away from every threshold of
    orbx_predict_scale_table, so another libm on another machine cannot move a level"""
    sc = _pair_scene(np.random.default_rng(4200 + seed), False, 4)
    for fma in (True, False):
        for p, res in zip(sc["problems"], sm.search(sc, fma, thr, scale_table())):
            for which, kf in ((1, p["kf1"]), (2, p["kf2"])):
                K = sc["keyframes"][kf]
                for i in np.nonzero(res["status%d" % which] >= sm.NO_CANDIDATE)[0]:
                    ratio = _ratio(sc, p, which, int(i))
                    assert all(abs(ratio - float(t)) > 1e-5 * float(t) for t in thr[1:NLEVELS] if np.isfinite(t)), "ratio on a threshold"
    return sc


def _ratio(sc, p, which, i):
    """mfMaxDistance / dist3D of feature i of side `which`, in float64 from the model's pose algebra"""
    sR12, sR21, t21 = sm.similarity(p["s12"], p["R12"], p["t12"])
    src = sc["keyframes"][p["kf1"] if which == 1 else p["kf2"]]
    T = np.asarray(src["Tcw"], F).reshape(4, 4)
    a = sm.mat_vec(T[:3, :3], src["world_pos"][i]) + T[:3, 3]
    c = sm.mat_vec(sR21 if which == 1 else sR12, a) + (t21 if which == 1 else np.asarray(p["t12"], F))
    return float(src["max_distance"][i]) / float(np.sqrt((c.astype(np.float64) ** 2).sum()))


# ------------------------------------------------------------------------------------------------ planted scenes
def _search(value, step, ok):
    """the float near `value` (within 8 ulps) for which ok holds"""
    v = F(value)
    for cand in [v] + [x for k in range(1, 9) for x in (_ulps(v, k), _ulps(v, -k))]:
        if ok(cand): return cand
    raise AssertionError("no float gives the planted product")


def _ulps(v, k):
    v = F(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf))
    return v


def planted_geometry():
    """the gates in front of the search; KF2 carries one keypoint (descriptor = the point's) under every projection that is
    meant to go on.  Returns the scene and {name: (feature of kf1, expected status)}"""
    rng = np.random.default_rng(4300)
    K1, K2 = KF(), KF()
    want = {}
    d0 = rnd_desc(rng)

    def plant(name, P, status, dmin=None, dmax=None, key=None):
        pt = point_at(P, d0, 0, dmin=dmin, dmax=dmax)
        i = K1.feat(5.0, 5.0 + len(K1.rows), 0, rnd_desc(rng), pt)
        if key is not None: K2.feat(key[0], key[1], 0, d0)
        want[name] = (i, status)

    # image bounds: u == maxx and v == maxy exactly are outside, u == minx and v == miny inside (x = +-1.25, y = +-0.9375 at z = 1)
    plant("u_eq_maxx", (1.25, 0.0, 1.0), sm.OUTSIDE)
    plant("u_eq_minx", (-1.25, 0.0, 1.0), sm.MATCH, key=(1.0, CY))
    plant("v_eq_maxy", (0.0, 0.9375, 1.0), sm.OUTSIDE)
    plant("v_eq_miny", (0.0, -0.9375, 1.0), sm.MATCH, key=(CX, 1.0))
    # depth sign: z = 0 goes on to invz = inf and fails IsInImage; slightly negative is rejected by the depth test.  (A world z
    # of -0 reaches the comparison as +0: the double accumulator of the matrix product starts at +0.0, in the reference as here.)
    plant("z_plus_zero", (0.5, 0.25, 0.0), sm.OUTSIDE)
    plant("z_minus_zero", (0.5, 0.25, -0.0), sm.OUTSIDE)
    plant("z_negative", (0.5, 0.25, -1e-6), sm.BEHIND)
    # distance band: dist3D = 2 (the point (0, 0, 2), projecting to the principal point)
    two = F(2.0)
    K2.feat(CX + 0.5, CY, 0, d0)
    lo_eq = _search(2.0 / 0.8, 1, lambda m: F(F(0.8) * m) == two)
    lo_out = _search(2.0 / 0.8, 1, lambda m: F(F(0.8) * m) == _ulps(two, 1))
    hi_eq = _search(2.0 / 1.2, 1, lambda m: F(F(1.2) * m) == two)
    hi_out = _search(2.0 / 1.2, 1, lambda m: F(F(1.2) * m) == _ulps(two, -1))
    plant("dist_eq_min", (0.0, 0.0, 2.0), sm.MATCH, dmin=lo_eq, dmax=F(2.0))
    plant("dist_below_min", (0.0, 0.0, 2.0), sm.DISTANCE, dmin=lo_out, dmax=F(4.0))
    plant("dist_eq_max", (0.0, 0.0, 2.0), sm.MATCH, dmin=F(0.1), dmax=hi_eq)
    plant("dist_above_max", (0.0, 0.0, 2.0), sm.DISTANCE, dmin=F(0.1), dmax=hi_out)
    k1, k2 = K1.build(), K2.build()
    return scene([k1, k2], [problem(0, 1, len(k1["keys_un"]), len(k2["keys_un"]))]), want


def planted_selection():
    """the level band, the descriptor threshold, ties, wide buckets and windows, clipped and empty windows, the mutual test.
    Returns the scene and {name: (side, feature, expected status, expected best)}"""
    rng = np.random.default_rng(4400)
    K1, K2 = KF(), KF()
    want = {}
    sf = scale_table()

    def query(name, u, v, level, desc, status, best=-1, side=1):
        src = K1 if side == 1 else K2
        i = src.feat(630.0, 2.0 + len(src.rows), 7, rnd_desc(rng), point_at(at_pixel(u, v), desc, level))
        want[name] = (side, i, status, best)
        return i

    # level band [pred - 1, pred]: four keypoints, octaves pred - 2 .. pred + 1, the ones outside the band closest in Hamming
    for name, pred, u in (("band_mid", 3, 60.0), ("band_level0", 0, 120.0), ("band_top", NLEVELS - 1, 200.0)):
        d = rnd_desc(rng)
        ids = {}
        for j, (oct_, nflip) in enumerate(((pred - 2, 0), (pred - 1, 30), (pred, 20), (pred + 1, 5))):
            if 0 <= oct_ < NLEVELS:
                ids[oct_] = K2.feat(u + j, 40.0, oct_, flips(rng, d, nflip))
        query(name, u + 1.0, 40.0, pred, d, sm.MATCH, ids[pred])
    d = rnd_desc(rng)                                                 # candidates only outside the band
    K2.feat(300.0, 40.0, 0, d); K2.feat(301.0, 40.0, 5, d)
    query("band_none", 300.5, 40.0, 3, d, sm.NO_CANDIDATE)
    # descriptor distance: exactly 100 is accepted, 101 is not
    for name, nflip, st, x in (("dist_100", 100, sm.MATCH, 400.0), ("dist_101", 101, sm.TOO_FAR, 460.0)):
        d = rnd_desc(rng)
        j = K2.feat(x, 40.0, 0, flips(rng, d, nflip))
        query(name, x + 0.5, 40.0, 0, d, st, j if st == sm.MATCH else -1)
    # two candidates at the same distance in different grid cells: the first visited (smaller ix) wins though its index is larger
    d = rnd_desc(rng)
    late = K2.feat(526.0, 40.0, 0, flips(rng, d, 12)); early = K2.feat(518.0, 40.0, 0, flips(rng, d, 12))
    assert sm.c_round(518.0 / 10) < sm.c_round(526.0 / 10) and early > late
    query("tie_first_visited", 522.0, 40.0, 0, d, sm.MATCH, early)
    # a bucket range of more than 64 items and a window of more than 64 candidates: 70 keypoints in one bucket, the best last
    d = rnd_desc(rng)
    wide = [K2.feat(100.5 + (j % 10) * 0.25, 120.5 + (j // 10) * 0.25, 0, flips(rng, d, 40 + j % 7)) for j in range(69)]
    wide.append(K2.feat(103.0, 122.5, 0, flips(rng, d, 3)))
    query("wide_window", 101.5, 121.5, 0, d, sm.MATCH, wide[-1])
    checks = dict(wide=(wide, 101.5, 121.5), clip={})
    # windows clipped at each image border, and an empty window
    for name, u, v in (("clip_left", 2.0, 200.0), ("clip_right", 637.0, 200.0), ("clip_top", 320.0, 2.0), ("clip_bottom", 320.0, 477.0)):
        d = rnd_desc(rng)
        j = K2.feat(min(u + 0.5, 634.0), min(v + 0.5, 474.0), 0, flips(rng, d, 7))   # (a keypoint past 634.9 / 474.9 is in no bucket)
        query(name, u, v, 0, d, sm.MATCH, j)
        checks["clip"][name] = (u, v)
    query("empty_window", 560.0, 300.0, 0, rnd_desc(rng), sm.NO_CANDIDATE)
    # mutual agreement.  a -> b and b -> a: a match.  a -> b with b -> a': none.  a -> b where b has no point: none.
    def mutual(name, u, back, matched2=False, b_point=True):
        d = rnd_desc(rng)
        a = K1.feat(u, 300.0, 0, flips(rng, d, 4), point_at(at_pixel(u, 300.0), d, 0))
        if back == "other":
            K1.feat(u + 3.0, 300.0, 0, d)                             # a': b's point is closer to it
        b = K2.feat(u + 0.5, 300.0, 0, flips(rng, d, 2), point_at(at_pixel(u, 300.0), d, 0) if b_point else None)
        want[name] = (1, a, sm.MATCH, b)
        return a, b
    a_ok, b_ok = mutual("mutual_agree", 60.0, "same")
    a_o, b_o = mutual("mutual_other", 120.0, "other")
    a_n, b_n = mutual("mutual_no_point", 180.0, "same", b_point=False)
    a_m, b_m = mutual("mutual_matched2", 240.0, "same")
    holder = K1.feat(20.0, 420.0, 0, rnd_desc(rng), point_at(at_pixel(20.0, 420.0), rnd_desc(rng), 0))   # already matched with b_m's point
    k1, k2 = K1.build(), K2.build()
    _assert_windows(k2, checks)
    sc = scene([k1, k2], [problem(0, 1, len(k1["keys_un"]), len(k2["keys_un"]), pairs=[(holder, b_m)])])
    mutual_want = dict(mutual_agree=(a_ok, b_ok), mutual_other=(a_o, -1), mutual_no_point=(a_n, -1), mutual_matched2=(a_m, -1))
    return sc, want, mutual_want


def _assert_windows(k2, checks):
    """on the model's grid of KF2: the 70 keypoints share ONE bucket (a bucket range of more than 64 items) and more than 64 of
    them pass the window test; every clipped window's unclamped cell range leaves the grid on the side its name says"""
    import math
    cells, (minx, miny, winv, hinv) = sm.grid_of(k2["keys_un"], BOUNDS4)
    wide, u, v = checks["wide"]
    r = F(TH)
    home = [(ix, iy) for ix in range(sm.COLS) for iy in range(sm.ROWS) if wide[0] in cells[ix][iy]]
    assert len(home) == 1 and set(wide) <= set(cells[home[0][0]][home[0][1]]) and len(cells[home[0][0]][home[0][1]]) > 64
    inside = [i for i in wide if abs(F(k2["keys_un"]["x"][i] - F(u))) < r and abs(F(k2["keys_un"]["y"][i] - F(v))) < r]
    assert len(inside) > 64
    for name, (u, v) in checks["clip"].items():
        x0, x1 = math.floor(F(F(F(u) - minx - r) * winv)), math.ceil(F(F(F(u) - minx + r) * winv))
        y0, y1 = math.floor(F(F(F(v) - miny - r) * hinv)), math.ceil(F(F(F(v) - miny + r) * hinv))
        assert dict(clip_left=x0 < 0, clip_right=x1 > sm.COLS - 1, clip_top=y0 < 0, clip_bottom=y1 > sm.ROWS - 1)[name], name


def shapes_scene():
    """keyframes of 0, 1, 63, 64 and 65 features; a problem with every feature already matched; three problems sharing KF1 with
    different Sim3 and different matched1; kf1 == kf2"""
    rng = np.random.default_rng(4500)
    kfs = []
    for n in (65, 0, 1, 63, 64):
        K = KF()
        for i in range(n):
            u, v = 40.0 + 8.0 * (i % 13) + 0.25 * (i % 3), 60.0 + 9.0 * (i // 13)
            d = rnd_desc(rng)
            K.feat(u + 0.5, v, i % 2, flips(rng, d, 5), point_at(at_pixel(u, v), d, 1) if i % 5 else None)
        kfs.append(K.build())
    n = [len(k["keys_un"]) for k in kfs]
    every = [(i, -1) for i in range(n[0])]
    probs = [problem(0, 4, n[0], n[4], pairs=[(3, 3), (7, -1)]),
             problem(0, 3, n[0], n[3], s12=1.0, t12=(0.015625, 0.0, 0.0), pairs=[(11, 12)]),
             problem(0, 2, n[0], n[2], s12=0.5, R12=PERMS[1]),
             problem(0, 1, n[0], n[1]),
             problem(0, 0, n[0], n[0]),
             problem(0, 4, n[0], n[4], pairs=every)]
    return scene(kfs, probs)


def all_scenes(thr):
    pg, _ = planted_geometry()
    ps, _, _ = planted_selection()
    return dict(exact=exact_scene(), float=float_scene(thr), planted_geometry=pg, planted_selection=ps, shapes=shapes_scene())


def planted_checks(thr):
    """every planted item on the model alone, in both fp_modes"""
    sf = scale_table()
    for fma in (True, False):
        sc, want = planted_geometry()
        res = sm.search(sc, fma, thr, sf)[0]
        for name, (i, st) in want.items():
            assert res["status1"][i] == st, (name, int(res["status1"][i]), st)
        assert res["uv1"][want["u_eq_maxx"][0]][0] == F(W) and res["uv1"][want["u_eq_minx"][0]][0] == F(0)
        assert res["uv1"][want["v_eq_maxy"][0]][1] == F(H_) and res["uv1"][want["v_eq_miny"][0]][1] == F(0)
        sc, want, mutual = planted_selection()
        res = sm.search(sc, fma, thr, sf)[0]
        for name, (side, i, st, best) in want.items():
            assert res["status%d" % side][i] == st and res["best%d" % side][i] == best, (name, int(res["status%d" % side][i]), int(res["best%d" % side][i]))
        assert res["level1"][want["band_level0"][1]] == 0 and res["level1"][want["band_top"][1]] == NLEVELS - 1
        for name, (a, b) in mutual.items():
            assert res["matches"][a] == b, (name, int(res["matches"][a]), b)
        a, b = mutual["mutual_other"][0], want["mutual_other"][3]
        assert res["best2"][b] >= 0 and res["best2"][b] != a                      # b -> a'
        assert res["status2"][want["mutual_matched2"][3]] == sm.NOT_SEARCHED and res["status2"][want["mutual_no_point"][3]] == sm.NOT_SEARCHED


# ------------------------------------------------------------------------------------------------ the harness side
def play(H, sc):
    """builds the scene in harness H; returns (keyframe ids, per keyframe the MapPoint id of each slot or -1)"""
    S = Scene(H)
    ids, slots = [], []
    for K in sc["keyframes"]:
        n = len(K["keys_un"])
        kf = S.kf(K["keys_un"], K["desc"].reshape(-1, 32) if n else np.zeros((0, 32), np.uint8), Tcw=np.asarray(K["Tcw"], F).reshape(4, 4))
        sl = np.full(n, -1, np.int32)
        for i in np.nonzero(K["has_point"])[0]:
            sl[i] = S.mp(K["point_desc"][i], pos=K["world_pos"][i], dmin=K["min_distance"][i], dmax=K["max_distance"][i])
            S.observe(int(sl[i]), kf, int(i))
        ids.append(kf); slots.append(sl)
    return S, ids, slots


def harness_search(H, sc):
    """every problem of the scene through h_search_by_sim3, problem by problem: [(count, matches12 as kf2 feature indices)]"""
    S, ids, slots = play(H, sc)
    out = []
    for p in sc["problems"]:
        n1 = len(sc["keyframes"][p["kf1"]]["keys_un"])
        s2 = slots[p["kf2"]]
        given = np.full(max(n1, 1), -1, np.int32)
        for a, b in p["pairs"]:
            given[a] = s2[b] if b >= 0 else S.mp(np.zeros(32, np.uint8))
            assert given[a] >= 0
        got, cnt = given.copy(), i32()
        H("h_search_by_sim3", ids[p["kf1"]], ids[p["kf2"]], got, CF32(p["s12"]), np.ascontiguousarray(p["R12"], F),
          np.ascontiguousarray(p["t12"], F), CF32(p["th"]), cnt)
        back = {int(v): j for j, v in enumerate(s2) if v >= 0}
        m = np.array([back[int(got[i])] if got[i] != given[i] else -1 for i in range(n1)], np.int32).reshape(-1)
        out.append((int(cnt[0]), m))
    return out


def driver_search(H, sc, batch):
    """every problem of the scene (all share kf1) through cs_search_by_sim3 of tests/compat_sim3search/driver.cpp: ONE
    ORBmatcher::SearchBySim3Batch call (batch) or the loop of single SearchBySim3 calls: [(count, matches12 as kf2 feature indices)]"""
    S, ids, slots = play(H, sc)
    P = sc["problems"]
    kf1 = P[0]["kf1"]
    assert all(p["kf1"] == kf1 for p in P)
    n1, K = len(sc["keyframes"][kf1]["keys_un"]), len(P)
    given = np.full((K, max(n1, 1)), -1, np.int32)
    for k, p in enumerate(P):
        for a, b in p["pairs"]:
            given[k, a] = slots[p["kf2"]][b] if b >= 0 else S.mp(np.zeros(32, np.uint8))
    got, cnt = np.ascontiguousarray(given[:, :n1]).copy(), i32(K)
    H("cs_search_by_sim3", ids[kf1], np.array([ids[p["kf2"]] for p in P], np.int32), K, got, np.array([p["s12"] for p in P], F),
      np.ascontiguousarray(np.stack([np.asarray(p["R12"], F).reshape(9) for p in P])), np.ascontiguousarray(np.stack([np.asarray(p["t12"], F) for p in P])),
      CF32(P[0]["th"]), int(batch), cnt)
    out = []
    for k, p in enumerate(P):
        back = {int(v): j for j, v in enumerate(slots[p["kf2"]]) if v >= 0}
        out.append((int(cnt[k]), np.array([back[int(got[k, i])] if got[k, i] != given[k, i] else -1 for i in range(n1)], np.int32).reshape(-1)))
    return out
