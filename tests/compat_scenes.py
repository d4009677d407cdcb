"""Scenes for the compat/ shims and the compiled reference matcher, shared by tests/test_compat_runtime.py and
tests/test_ref_matcher.py: the ctypes wrapper of a harness (tests/compat_runtime/harness.cpp and oracle/ref/matcher/harness.cpp
have the same extern "C" entry points), a Scene that builds a map in one, the Python model of the MapPoint rules, and the
generators of the scenes in which the six pose-algebra methods compute exactly."""
import ctypes as C
import math

import numpy as np

import oracle
from test_bow_policies import make_featvec, perturbed_copy, random_kf

KP = oracle.KP_DTYPE
F32 = C.c_float
W, H_, FX, CX, CY = 640, 480, 256.0, 320.0, 240.0
K4 = np.array([FX, FX, CX, CY], np.float32)


class HarnessError(RuntimeError):
    pass


class Harness:
    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.h_error.restype = C.c_char_p

    def __call__(self, name, *args):
        conv = [a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else int(a) if isinstance(a, np.integer) else a for a in args]
        if getattr(self.L, name)(*conv) != 0:
            raise HarnessError(self.L.h_error().decode())


def i32(n=1):
    return np.zeros(n, np.int32)


def scale_tables(levels=8, f=1.2):
    sf = np.ones(levels, np.float32)
    for l in range(1, levels):
        sf[l] = np.float32(sf[l - 1] * np.float32(f))
    s2 = (sf * sf).astype(np.float32)
    return sf, s2, (np.float32(1.0) / s2).astype(np.float32)


class Scene:
    """A fresh map in the harness; keyframes, frames and points are addressed by the index the harness returns."""

    def __init__(self, H):
        self.H = H
        H("h_reset")
        H("h_set_frame_bounds", F32(0), F32(W), F32(0), F32(H_))
        self.kf_n = []
        self.nmp = 0

    def kf(self, keys, desc, u_right=None, Tcw=None, mbf=0.0, fv=None, K=K4):
        n = len(keys)
        ur = np.full(n, -1, np.float32) if u_right is None else np.ascontiguousarray(u_right, np.float32)
        T = np.eye(4, dtype=np.float32) if Tcw is None else np.ascontiguousarray(Tcw, np.float32)
        nodes, begin, index = oracle.orb_oracle._flat_featvec(fv or {})
        out = i32()
        self.H("h_add_keyframe", n, np.ascontiguousarray(keys, KP), np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), ur, T,
               np.ascontiguousarray(K, np.float32), F32(mbf), np.array([0, W, 0, H_], np.int32), 8, F32(1.2), len(nodes),
               np.ascontiguousarray(nodes, np.uint32), np.ascontiguousarray(begin, np.int32), np.ascontiguousarray(index, np.uint32), out)
        self.kf_n.append(n)
        return int(out[0])

    def frame(self, keys, desc, u_right=None, Tcw=None, mb=0.0, mbf=0.0, fv=None, keys_raw=None, K=K4):
        n = len(keys)
        ur = np.full(n, -1, np.float32) if u_right is None else np.ascontiguousarray(u_right, np.float32)
        nodes, begin, index = oracle.orb_oracle._flat_featvec(fv or {})
        out = i32()
        k = np.ascontiguousarray(keys, KP)
        self.H("h_add_frame", n, k if keys_raw is None else np.ascontiguousarray(keys_raw, KP), k,
               np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), ur, None if Tcw is None else np.ascontiguousarray(Tcw, np.float32),
               np.ascontiguousarray(K, np.float32), F32(mb), F32(mbf), 8, F32(1.2), len(nodes), np.ascontiguousarray(nodes, np.uint32),
               np.ascontiguousarray(begin, np.int32), np.ascontiguousarray(index, np.uint32), out)
        return int(out[0])

    def mp(self, desc, pos=(0.0, 0.0, 1.0), normal=(0.0, 0.0, 1.0), dmin=0.5, dmax=4.0):
        out = i32()
        self.H("h_add_mappoint", np.array(pos, np.float32), np.array(normal, np.float32), np.ascontiguousarray(desc, np.uint8),
               F32(dmin), F32(dmax), out)
        self.nmp += 1
        return int(out[0])

    def observe(self, mp, kf, idx):
        self.H("h_observe", mp, kf, idx)

    def slots(self, kf):
        out = i32(max(self.kf_n[kf], 1))
        self.H("h_kf_slots", kf, out)
        return out[:self.kf_n[kf]].copy()

    def state(self, mp):
        bad, nobs, ne = i32(), i32(), i32()
        d = np.zeros(32, np.uint8); ok, oi = i32(64), i32(64)
        self.H("h_mp_state", mp, bad, nobs, d, ok, oi, 64, ne)
        return bool(bad[0]), int(nobs[0]), d.tobytes(), tuple(zip(ok[:ne[0]].tolist(), oi[:ne[0]].tolist()))

    def map_state(self):
        return [self.slots(k).tolist() for k in range(len(self.kf_n))], [self.state(i) for i in range(self.nmp)]


def flips(rng, d, nbits):
    d = np.array(d, np.uint8).copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def hamming(a, b):
    a, b = (np.frombuffer(x, np.uint8) if isinstance(x, bytes) else np.asarray(x, np.uint8) for x in (a, b))
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


class PyPoint:
    """Python model of the map rules restated in tests/compat_runtime/MapPoint.h"""

    def __init__(self, desc):
        self.desc, self.obs, self.nobs, self.bad = bytes(desc), {}, 0, False


def py_add_obs(p, kf, idx, u_right):
    if kf in p.obs:
        return
    p.obs[kf] = idx
    p.nobs += 2 if u_right[kf][idx] >= 0 else 1


def py_best_descriptor(rows):
    n = len(rows)
    D = np.array([[hamming(rows[i], rows[j]) for j in range(n)] for i in range(n)])
    med = np.sort(D, axis=1)[:, (n - 1) // 2]
    return bytes(rows[int(np.argmin(med))])                           # argmin: the first of equal medians


def py_replace(pts, slots, descs, u_right, i, j):
    p, q = pts[i], pts[j]
    if i == j:
        return
    obs, p.obs, p.bad = dict(p.obs), {}, True
    for kf in sorted(obs):
        if kf not in q.obs:
            slots[kf][obs[kf]] = j
            py_add_obs(q, kf, obs[kf], u_right)
        else:
            slots[kf][obs[kf]] = -1
    if not q.bad and q.obs:
        q.desc = bytes(py_best_descriptor([descs[kf][q.obs[kf]] for kf in sorted(q.obs)]))


def _frame_with_points(S, rng, keys, desc, p_slot=0.25, p_bad=0.1):
    """a frame whose features partly already carry map points (some bad, some observed once or twice)"""
    n = len(keys)
    f = S.frame(keys, desc)
    holder = S.kf(np.zeros(n, KP), desc)
    holder2 = S.kf(np.zeros(n, KP), desc)
    slot_mp = np.full(n, -1, np.int32)
    for i in np.nonzero(rng.uniform(size=n) < p_slot)[0]:
        p = S.mp(desc[i])
        r = rng.integers(0, 3)
        if r >= 1: S.observe(p, holder, int(i))
        if r >= 2: S.observe(p, holder2, int(i))
        S.H("h_frame_set", f, int(i), p, 0)
        slot_mp[i] = p
    return f, slot_mp


def _bow_keyframe(S, rng, kf, p_bad=0.1):
    """kf (random_kf / perturbed_copy layout) into the harness with a MapPoint per has_map_point slot, some of them bad;
    returns the keyframe, its slots and the has_map_point the policies see (bad = absent)"""
    k = S.kf(kf["keys_un"], kf["desc"], kf["u_right"], fv=kf["feat_vec"])
    for i in np.nonzero(kf["has_map_point"])[0]:
        p = S.mp(kf["desc"][i])
        S.observe(p, k, int(i))
        if rng.uniform() < p_bad:
            S.H("h_set_bad", p)                                      # erases its slot ...
            if rng.uniform() < 0.5:
                S.observe(S.mp(kf["desc"][i]), k, int(i))            # ... which another point may take
    slots = S.slots(k)
    return k, slots


# Scenes in which the shims' float pose algebra is exact.  A point is placed by its camera coordinates xc = (a, b, c) * 2^e with
# a^2 + b^2 + c^2 = d^2 (c a power of two larger than |a|, |b|): the projection (fx = 256) and the distance d * 2^e are exact;
# mfMaxDistance = dist * 1.2^(L - 1/2), so PredictScale gives L with half a level to spare.

QUADS = [(a, b, c, int(math.isqrt(a * a + b * b + c * c))) for c in (32, 64, 128) for a in range(0, c // 2) for b in range(0, c // 2)
         if math.isqrt(a * a + b * b + c * c) ** 2 == a * a + b * b + c * c]
PERMS = [np.eye(3, dtype=np.float32), np.eye(3, dtype=np.float32)[[1, 0, 2]], np.eye(3, dtype=np.float32)[[2, 0, 1]]]


def exact_camera_point(rng):
    a, b, c, d = QUADS[rng.integers(0, len(QUADS))]
    a, b = (a, b) if rng.uniform() < 0.5 else (b, a)
    e = 2.0 ** int(rng.integers(-5, -1))
    xc = np.array([a * rng.choice([-1, 1]), b * rng.choice([-1, 1]), c], np.float64) * e
    return xc, d * e


def project(xc):
    return np.float32(FX * (xc[0] / xc[2]) + CX), np.float32(FX * (xc[1] / xc[2]) + CY)


def add_exact_point(S, rng, R, t, xc, dist, desc, level):
    """a MapPoint with camera coordinates xc in the camera [R | t]: world position R^T (xc - t)"""
    X = (R.astype(np.float64).T @ (xc - t.astype(np.float64)))
    assert np.array_equal(X.astype(np.float32).astype(np.float64), X)
    dmax = np.float32(dist * 1.2 ** (level - 0.5))
    o = X - (-R.astype(np.float64).T @ t)
    return S.mp(desc, pos=X, normal=(o / dist).astype(np.float32), dmin=dmax / np.float32(1.2 ** 7), dmax=dmax)


def keys_near(rng, uv, levels, n_extra, spread=4, dlevel=(0, 2)):
    """a keypoint near each projection (within spread / 4 pixels; octave = predicted level minus dlevel[0] ... dlevel[1] - 1) and
    distractors"""
    n = len(uv) + n_extra
    k = np.zeros(n, KP)
    k["x"][:len(uv)] = uv[:, 0] + rng.integers(-spread, spread + 1, len(uv)) / 4.0
    k["y"][:len(uv)] = uv[:, 1] + rng.integers(-spread, spread + 1, len(uv)) / 4.0
    k["octave"][:len(uv)] = np.clip(levels - rng.integers(dlevel[0], dlevel[1], len(uv)), 0, 7)
    k["x"][len(uv):] = rng.uniform(10, W - 10, n_extra); k["y"][len(uv):] = rng.uniform(10, H_ - 10, n_extra)
    k["octave"][len(uv):] = rng.integers(0, 8, n_extra)
    k["angle"] = rng.uniform(0, 360, n)
    perm = rng.permutation(n)
    return k[perm], perm


def target_dict(keys, desc, u_right=None):
    sf, s2, is2 = scale_tables()
    return dict(keys_un=keys, desc=desc, bounds=(0.0, float(W), 0.0, float(H_)), scale_factors=sf, inv_level_sigma2=is2,
                level_sigma2=s2, u_right=np.full(len(keys), -1, np.float32) if u_right is None else u_right)


def exact_scene(S, rng, R, t, npts, mbf=0.0, n_extra=60, p_key=0.8):
    """npts points seen by the camera [R | t] and a keyframe (pose [R | t]) with keypoints near most of their projections"""
    xcs, ds, levels, descs = [], [], [], []
    for _ in range(npts):
        xc, dist = exact_camera_point(rng)
        xcs.append(xc); ds.append(dist); levels.append(int(rng.integers(1, 7))); descs.append(rng.integers(0, 256, 32, dtype=np.uint8))
    uv = np.array([project(x) for x in xcs], np.float32)
    levels = np.array(levels, np.int32)
    seen = np.nonzero(rng.uniform(size=npts) < p_key)[0]
    keys, perm = keys_near(rng, uv[seen], levels[seen], n_extra)
    kdesc = np.zeros((len(keys), 32), np.uint8)
    src = np.concatenate([seen, np.full(n_extra, -1)])[perm]
    for j, i in enumerate(src):
        kdesc[j] = flips(rng, descs[i], int(rng.integers(0, 30))) if i >= 0 else rng.integers(0, 256, 32, dtype=np.uint8)
    ur = np.where(rng.uniform(size=len(keys)) < 0.4, keys["x"] - rng.integers(1, 40, len(keys)), -1).astype(np.float32)
    Tcw = np.eye(4, dtype=np.float32); Tcw[:3, :3] = R; Tcw[:3, 3] = t
    kf = S.kf(keys, kdesc, ur, Tcw=Tcw, mbf=mbf)
    ids = [add_exact_point(S, rng, R, t, xcs[i], ds[i], descs[i], levels[i]) for i in range(npts)]
    pts = dict(uv=uv, level=levels, desc=np.array(descs), u_right=(uv[:, 0] - np.float32(mbf) / np.array([x[2] for x in xcs], np.float32)).astype(np.float32),
               angle=np.zeros(npts, np.float32))
    return kf, np.array(ids, np.int32), pts, target_dict(keys, kdesc, ur)


def pose(R, t):
    T = np.eye(4, dtype=np.float32); T[:3, :3] = R; T[:3, 3] = t
    return T


def _triangulation_scene(S, rng, nneigh, plant=None):
    """kf1 (pose [I | (-1, -2, 0)]) and neighbours of pose [swap-xy | (2, -1, 1/4)]: the epipole C2 = (4, 0, 1/4) is exact;
    F12 maps a point to the horizontal line through it, along which perturbed_copy moves the features"""
    base = random_kf(rng, 400, p_mp=0.3)
    base["feat_vec"] = make_featvec(base["desc"])
    if plant: plant("base", base)
    T1 = pose(np.eye(3, dtype=np.float32), np.array([-1, -2, 0], np.float32))
    T2 = pose(PERMS[1], np.array([2, -1, 0.25], np.float32))
    kf1 = S.kf(base["keys_un"], base["desc"], base["u_right"], Tcw=T1, fv=base["feat_vec"])
    for i in np.nonzero(base["has_map_point"])[0]: S.observe(S.mp(base["desc"][i]), kf1, int(i))
    neigh = []
    for _ in range(nneigh):
        kf = perturbed_copy(rng, base, nflip=int(rng.integers(4, 12)))
        kf["feat_vec"] = make_featvec(kf["desc"])
        if plant: plant("neighbour", kf)
        k = S.kf(kf["keys_un"], kf["desc"], kf["u_right"], Tcw=T2, fv=kf["feat_vec"])
        for i in np.nonzero(kf["has_map_point"])[0]: S.observe(S.mp(kf["desc"][i]), k, int(i))
        neigh.append((k, kf))
    F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    return base, kf1, neigh, F12, (FX * 4 * 4 + CX, CY)


def _fuse_scene(S, rng):
    """two target keyframes a, b (same camera), list members p_i and p_j with p_j in a's slot s:
    at a, p_i matches slot s and, observed less, is replaced by p_j (p_i->Replace(p_j)); p_j takes p_i's observations and its
    descriptor becomes B; at b, p_j then matches the B keypoint instead of the A keypoint.  Plus ordinary points, a repeated
    pointer and NULL entries."""
    A = rng.integers(0, 256, 32, dtype=np.uint8)
    B = flips(rng, A, 30)
    X = rng.integers(0, 256, 32, dtype=np.uint8)
    R, t = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    xc, dist = np.array([4.0, 8.0, 64.0]) / 64, 72.0 / 64            # (4, 8, 64) has norm 72
    u, v = project(xc)
    nrm = 40
    others = [exact_camera_point(rng) for _ in range(nrm)]
    ouv = np.array([project(x) for x, _ in others], np.float32)
    odesc = rng.integers(0, 256, (nrm, 32), dtype=np.uint8)

    def kf_keys(extra):
        k = np.zeros(len(extra) + nrm, KP)
        for j, (x, y, o) in enumerate(extra):
            k[j]["x"], k[j]["y"], k[j]["octave"] = x, y, o
        k["x"][len(extra):] = ouv[:, 0] + 0.25; k["y"][len(extra):] = ouv[:, 1]; k["octave"][len(extra):] = 1
        return k
    # keyframe a: slot 0 = the keypoint p_j was seen at (descriptor A, stereo); b: slot 0 the A keypoint, slot 1 the B keypoint
    ka = kf_keys([(u + 0.5, v, 1)]); da = np.vstack([A[None], [flips(rng, d, 3) for d in odesc]])
    kb = kf_keys([(u + 0.5, v, 1), (u - 0.5, v + 0.25, 1)]); db = np.vstack([A[None], B[None], [flips(rng, d, 5) for d in odesc]])
    ura = np.full(len(ka), -1, np.float32); ura[0] = u
    a = S.kf(ka, da, ura); b = S.kf(kb, db)
    c = S.kf(np.zeros(1, KP), X[None], np.zeros(1, np.float32))     # p_j's second, stereo observation
    ds = [S.kf(np.zeros(1, KP), B[None]) for _ in range(3)]          # p_i's three mono observations
    lvl = 1
    pj = add_exact_point(S, rng, R, t, xc, dist, A, lvl)
    S.observe(pj, a, 0); S.observe(pj, c, 0)                          # Observations() = 4
    pi = add_exact_point(S, rng, R, t, xc, dist, B, lvl)
    for d in ds: S.observe(pi, d, 0)                                   # Observations() = 3
    ords = [add_exact_point(S, rng, R, t, others[q][0], others[q][1], odesc[q], 1) for q in range(nrm)]
    for q in range(0, nrm, 4): S.observe(S.mp(odesc[q]), a, 1 + q)   # some of a's slots already hold (fewer-observed) points
    lst = [pi, -1, pj] + ords[:10] + [ords[3], -1] + ords[10:]
    return dict(a=a, b=b, pi=pi, pj=pj, A=A, B=B, list=np.array(lst, np.int32), kfs=np.array([a, b], np.int32))
