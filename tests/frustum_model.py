"""numpy restatement of the frustum stage in front of the batched map-point matcher (csrc/orbx_kernels.hip: k_track_frustum;
include/orbx.h: orbx_search_local_points_batch_device, orbx_predict_scale_table): Frame::isInFrustum (reference
src/Frame.cc:529-620), MapPoint::PredictScale (src/MapPoint.cc:706-721) and the first lines of SearchByProjection(F,
vpMapPoints, th) (src/ORBmatcher.cc:82-101, 187-194), in float32 / float64 with one scalar step per line, plus the seeded
scenes the CPU and GPU tests share.

The logarithm is libm's logf, called through ctypes: np.log's float32 path is not glibc's.  The fused steps of ORBX_FP_GCC_FMA
are libm's fmaf (one rounding); a float64 product-and-sum rounded to float32 would round twice.
"""
import ctypes
import ctypes.util

import numpy as np

import track_model as tm

F32, F64 = np.float32, np.float64
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float; _libm.logf.argtypes = [ctypes.c_float]
_libm.fmaf.restype = ctypes.c_float; _libm.fmaf.argtypes = [ctypes.c_float] * 3
GATES = ("in view", "depth", "u", "v", "near", "far", "cos")    # `gate`: the test that switched a point off; -1 = skipped


def logf(x):
    return F32(_libm.logf(float(x)))


def fmaf(a, b, c):
    return F32(_libm.fmaf(float(a), float(b), float(c)))


def bits_to_f32(b):
    return np.array([b], np.uint32).view(F32)[0]


def f32_to_bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


def step(x, n):
    """the float n places after (n < 0: before) the positive finite float x"""
    return bits_to_f32(f32_to_bits(x) + n)


# ------------------------------------------------------------------------------------------------ PredictScale
def raw_scale(ratio, log_scale_factor):
    """(int)ceilf(logf(ratio) / mfLogScaleFactor) before the clamp, for a positive finite ratio"""
    q = F32(logf(F32(ratio)) / F32(log_scale_factor))
    return int(np.ceil(q))


def clamped_scale(max_distance, current_dist, scale_factor, nlevels):
    """tests/compat_runtime/map_model.cpp: ClampedScale, with libm's logf; the ratio must be positive and finite"""
    ratio = F32(F32(max_distance) / F32(current_dist))
    n = raw_scale(ratio, logf(F32(scale_factor)))
    return 0 if n < 0 else nlevels - 1 if n >= nlevels else n


def predict_scale_table(scale_factor, nlevels):
    """thr[k] = the smallest positive finite float whose raw scale is >= k (+inf: none); thr[0] = 0"""
    lsf = logf(F32(scale_factor))
    thr = np.zeros(nlevels, F32)
    for k in range(1, nlevels):
        lo, hi = 0x00000001, 0x7f7fffff
        if raw_scale(bits_to_f32(hi), lsf) < k:
            thr[k] = np.inf
            continue
        assert raw_scale(bits_to_f32(lo), lsf) < k
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if raw_scale(bits_to_f32(mid), lsf) >= k:
                hi = mid
            else:
                lo = mid
        thr[k] = bits_to_f32(hi)
    return thr


def table_level(thr, ratio):
    """the number of k >= 1 with ratio >= thr[k]: NaN and <= 0 give 0, +inf gives nlevels - 1"""
    with np.errstate(invalid="ignore"):
        return int(sum(1 for k in range(1, len(thr)) if F32(ratio) >= thr[k]))


# ------------------------------------------------------------------------------------------------ the stage
def _gemm3(a, b, c):
    t = F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))
    return F32(F64(t) + F64(c))


def frustum(problem, pool, scale, thr, fma, camera=tm.CAMERA, bounds=tm.BOUNDS, mbf=tm.MBF):
    """per listed point of `problem`: in_view, the five tracking fields (where in view), the DTrackQ window x, y, ur, r,
    min_level, max_level (r = -1, levels -1, zeros where switched off) and the gate that switched it off"""
    fx, fy, cx, cy = (F32(v) for v in camera)
    minx, maxx, miny, maxy = (F32(v) for v in bounds)
    mbf = F32(mbf)
    T = np.asarray(problem["Tcw"], F32).reshape(4, 4)
    Rcw, tcw = T[:3, :3], T[:3, 3]
    Ow = np.asarray(problem["Ow"], F32)
    th, limit = F32(problem["th"]), F32(problem.get("viewing_cos_limit", 0.5))
    index = problem.get("point_index")
    index = np.arange(len(pool["world_pos"]), dtype=np.int32) if index is None else np.asarray(index, np.int32)
    skip = problem.get("skip")
    n = len(index)
    out = dict(in_view=np.zeros(n, np.uint8), proj_x=np.zeros(n, F32), proj_y=np.zeros(n, F32), proj_xr=np.zeros(n, F32),
               view_cos=np.zeros(n, F32), level=np.zeros(n, np.int32), x=np.zeros(n, F32), y=np.zeros(n, F32), ur=np.zeros(n, F32),
               r=np.full(n, -1.0, F32), min_level=np.full(n, -1, np.int32), max_level=np.full(n, -1, np.int32),
               gate=np.zeros(n, np.int32), index=index)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i, pi in enumerate(index):
            if skip is not None and skip[i]:
                out["gate"][i] = -1                                     # skipped by the caller: not a gate of isInFrustum
                continue
            P = pool["world_pos"][pi].astype(F32)
            Pn = pool["normal"][pi].astype(F32)
            PcX = _gemm3(Rcw[0], P, tcw[0])
            PcY = _gemm3(Rcw[1], P, tcw[1])
            PcZ = _gemm3(Rcw[2], P, tcw[2])
            if PcZ < F32(0.0):
                out["gate"][i] = 1; continue
            invz = F32(F32(1.0) / PcZ)
            if fma:
                u = fmaf(F32(fx * PcX), invz, cx)
                v = fmaf(F32(fy * PcY), invz, cy)
            else:
                u = F32(F32(F32(fx * PcX) * invz) + cx)
                v = F32(F32(F32(fy * PcY) * invz) + cy)
            if u < minx or u > maxx:
                out["gate"][i] = 2; continue
            if v < miny or v > maxy:
                out["gate"][i] = 3; continue
            maxDistance = F32(F32(1.2) * F32(pool["max_distance"][pi]))
            minDistance = F32(F32(0.8) * F32(pool["min_distance"][pi]))
            POx = F32(P[0] - Ow[0])
            POy = F32(P[1] - Ow[1])
            POz = F32(P[2] - Ow[2])
            s2 = F64(0.0)
            s2 = s2 + F64(POx) * F64(POx)
            s2 = s2 + F64(POy) * F64(POy)
            s2 = s2 + F64(POz) * F64(POz)
            dist = F32(np.sqrt(s2))
            if dist < minDistance:
                out["gate"][i] = 4; continue
            if dist > maxDistance:
                out["gate"][i] = 5; continue
            dot = F64(0.0)
            dot = dot + F64(POx) * F64(Pn[0])
            dot = dot + F64(POy) * F64(Pn[1])
            dot = dot + F64(POz) * F64(Pn[2])
            viewCos = F32(dot / F64(dist))
            if viewCos < limit:
                out["gate"][i] = 6; continue
            ratio = F32(F32(pool["max_distance"][pi]) / dist)
            level = table_level(thr, ratio)
            ur = fmaf(-mbf, invz, u) if fma else F32(u - F32(mbf * invz))
            r = F32(2.5) if F64(viewCos) > 0.998 else F32(4.0)
            if float(th) != 1.0:
                r = F32(r * th)
            r = F32(r * scale[level])
            out["in_view"][i] = 1
            out["proj_x"][i], out["proj_y"][i], out["proj_xr"][i], out["view_cos"][i], out["level"][i] = u, v, ur, viewCos, level
            out["x"][i], out["y"][i], out["ur"][i], out["r"][i] = u, v, ur, r
            out["min_level"][i], out["max_level"][i] = level - 1, level
    return out


def as_mp_problem(problem, pool, st, cap=None):
    """the model's fields as the problem dict tests/track_model.py and the existing map-point calls take"""
    idx = st["index"]
    fo = problem.get("frame_observations")
    return dict(th=F32(problem["th"]), frame_observations=fo, in_view=st["in_view"].copy(),
                proj=np.stack([st["proj_x"], st["proj_y"], st["proj_xr"]], 1).astype(F32), level=st["level"].copy(),
                view_cos=st["view_cos"].copy(), mp_desc=np.ascontiguousarray(pool["mp_desc"][idx]).reshape(-1, 32),
                observations=np.ascontiguousarray(pool["observations"][idx]).astype(np.int32))


# ------------------------------------------------------------------------------------------------ scenes
def camera_centre(Tcw):
    T = np.asarray(Tcw, F64)
    return (-T[:3, :3].T @ T[:3, 3]).astype(F32)


def make_pool(rng, frame, M, Tcw, scale_factor=1.2):
    """M local-map points that project near features of `frame` under Tcw, at all pyramid levels, and fodder for every gate"""
    fx, fy, cx, cy = tm.CAMERA
    kf, n = frame["keys"], len(frame["keys"])
    T = np.asarray(Tcw, F64)
    R, t = T[:3, :3], T[:3, 3]
    Ow = -R.T @ t
    if n > 0:
        src = rng.integers(0, n, M)
        u = kf["x"][src] + rng.normal(0, 1.0, M)
        v = kf["y"][src] + rng.normal(0, 1.0, M)
        z = frame["depth"][src] * (1 + rng.normal(0, 0.01, M))
        desc = frame["desc"][src].copy()
        oct_ = kf["octave"][src].astype(int)
    else:
        u, v, z = rng.uniform(0, 200, M), rng.uniform(0, 150, M), rng.uniform(1, 10, M)
        desc = rng.integers(0, 256, (M, 32), dtype=np.uint8)
        oct_ = rng.integers(0, 8, M)
    kind = rng.choice(7, M, p=[.64, .06, .06, .06, .06, .06, .06])   # 0 = meant to be seen, 1 .. 6 = fodder for that gate
    z = np.where(kind == 1, -z, z)
    u = np.where(kind == 2, u + 500.0, u)
    v = np.where(kind == 3, v - 400.0, v)
    Xc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    xw = ((Xc - t) @ R).astype(F32)
    po = xw.astype(F64) - Ow
    dist = np.linalg.norm(po, axis=1)
    level = np.clip(oct_ + rng.integers(0, 2, M), 0, 7)               # the band [level - 1, level] then holds the feature's octave
    maxd = dist * scale_factor ** (level - 0.5)
    maxd = np.where(kind == 5, dist / 1.5, maxd)
    mind = maxd / scale_factor ** 7
    mind = np.where(kind == 4, dist * 1.5, mind)
    ang = rng.choice([0.0, 0.03, 0.1, 0.8], M)                         # cosines 1, 0.99955, 0.995, 0.70
    ang = np.where(kind == 6, 1.3, ang)                                # 0.27
    d0 = po / np.maximum(dist, 1e-9)[:, None]
    side = np.cross(d0, rng.normal(size=(M, 3)))
    side /= np.maximum(np.linalg.norm(side, axis=1), 1e-9)[:, None]
    normal = (np.cos(ang)[:, None] * d0 + np.sin(ang)[:, None] * side).astype(F32)
    for row in desc:
        for b in rng.integers(0, 256, rng.integers(0, 3)):
            row[b >> 3] ^= np.uint8(1 << (b & 7))
    return dict(world_pos=xw, normal=normal, min_distance=mind.astype(F32), max_distance=maxd.astype(F32), mp_desc=desc,
                observations=rng.choice([0, 1, 2], M).astype(np.int32))


def make_problem(rng, frame_id, Tcw, M, cap, th=3.0, jitter=0.01, subset=True, occupied=0.2):
    """one problem on a pool of M points: the pool's pose moved a little, a permuted subset of the pool, some points skipped"""
    T = np.asarray(Tcw, F64).copy()
    T[:3, 3] += rng.normal(0, jitter, 3)
    if subset:
        index = rng.permutation(M)[:max(1, int(M * rng.uniform(0.6, 1.0)))].astype(np.int32)
    else:
        index = None
    npts = M if index is None else len(index)
    fo = np.where(rng.uniform(size=cap) < occupied, rng.integers(1, 5, cap), rng.choice([-1, 0], cap)).astype(np.int32)
    return dict(frame=frame_id, th=F32(th), viewing_cos_limit=F32(0.5), Tcw=T.astype(F32), Ow=camera_centre(T.astype(F32)),
                point_index=index, skip=(rng.uniform(size=npts) < 0.1).astype(np.uint8), frame_observations=fo)
