"""ORBmatcher::SearchBySim3 (reference src/ORBmatcher.cc:1433-1684) restated in numpy float32 / float64, independently of
csrc/orbx_sim3search.h, under the arithmetic of the stand-in cv::Mat (tests/compat_runtime/opencv2/core/core.hpp): scalar * Mat
element-wise through double, matrix products with a double accumulator rounded once, + and unary - in float, cv::norm as the
square root of a double sum.  u = fx x + cx and v = fy y + cy are one fmaf under FP_GCC_FMA and two roundings under FP_STRICT.
The level is the count of thresholds of orbx_predict_scale_table the ratio reaches.  KeyFrame::GetFeaturesInArea is the bucket
walk of the Frame grid: 64 x 48 buckets, ix outer, iy inner, features of a bucket in ascending index.

search(scene, fma, thr, scale) returns per problem a dict: n, matches, status1/2, best1/2, level1/2, uv1/2."""
import math

import numpy as np

from frustum_model import fmaf

F32, F64 = np.float32, np.float64
NOT_SEARCHED, BEHIND, OUTSIDE, DISTANCE, NO_CANDIDATE, TOO_FAR, MATCH = range(7)
COLS, ROWS, TH_HIGH = 64, 48, 100


def mat_vec(M, p):
    out = np.zeros(3, F32)
    for i in range(3):
        s = F64(0.0)
        for k in range(3):
            s = s + F64(M[i, k]) * F64(p[k])
        out[i] = F32(s)
    return out


def similarity(s12, R12, t12):
    R12 = np.asarray(R12, F32).reshape(3, 3)
    s, inv = F64(F32(s12)), F64(1.0) / F64(F32(s12))
    sR12 = (R12.astype(F64) * s).astype(F32)
    sR21 = (R12.T.astype(F64) * inv).astype(F32)
    t21 = mat_vec(-sR21, np.asarray(t12, F32))
    return sR12, sR21, t21


def level_of(thr, nlevels, ratio):
    return int(sum(1 for k in range(1, nlevels) if ratio >= thr[k]))


def project(P, Rw, tw, sR, t, cam, bounds, th, dmin, dmax, fma, thr, scale):
    """-> status (BEHIND .. DISTANCE, or NO_CANDIDATE = goes on to the search), u, v, level, radius"""
    with np.errstate(all="ignore"):
        a = mat_vec(Rw, P) + tw
        c = mat_vec(sR, a) + t
        if F64(c[2]) < 0.0:
            return BEHIND, F32(0), F32(0), -1, None
        invz = F32(F64(1.0) / F64(c[2]))
        x, y = F32(c[0] * invz), F32(c[1] * invz)
        fx, fy, cx, cy = (F32(v) for v in cam)
        if fma:
            u, v = fmaf(fx, x, cx), fmaf(fy, y, cy)
        else:
            u, v = F32(F32(fx * x) + cx), F32(F32(fy * y) + cy)
        minx, maxx, miny, maxy = (F32(b) for b in bounds)
        if not (u >= minx and u < maxx and v >= miny and v < maxy):
            return OUTSIDE, u, v, -1, None
        s2 = F64(0.0)
        for k in range(3):
            s2 = s2 + F64(c[k]) * F64(c[k])
        dist = F32(np.sqrt(s2))
        if dist < F32(F32(0.8) * F32(dmin)) or dist > F32(F32(1.2) * F32(dmax)):
            return DISTANCE, u, v, -1, None
        level = level_of(thr, len(scale), F32(F32(dmax) / dist))
        return NO_CANDIDATE, u, v, level, F32(F32(th) * F32(scale[level]))


def grid_of(keys, bounds):
    minx, maxx, miny, maxy = (F32(b) for b in bounds)
    winv, hinv = F32(F32(64.0) / F32(maxx - minx)), F32(F32(48.0) / F32(maxy - miny))
    cells = [[[] for _ in range(ROWS)] for _ in range(COLS)]
    for i in range(len(keys)):
        px = c_round(F32(F32(keys["x"][i] - minx) * winv)); py = c_round(F32(F32(keys["y"][i] - miny) * hinv))
        if 0 <= px < COLS and 0 <= py < ROWS:
            cells[px][py].append(i)
    return cells, (minx, miny, winv, hinv)


def c_round(v):
    """C round(): half away from zero"""
    v = float(v)
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def best_in_area(grid, keys, desc, u, v, r, level, qdesc):
    """GetFeaturesInArea(u, v, r) + the loop of :1555-1573: (index of the first strict minimum or -1, its distance)"""
    cells, (minx, miny, winv, hinv) = grid
    x0 = max(0, int(math.floor(F32(F32(F32(u - minx) - r) * winv)))); x1 = min(COLS - 1, int(math.ceil(F32(F32(F32(u - minx) + r) * winv))))
    y0 = max(0, int(math.floor(F32(F32(F32(v - miny) - r) * hinv)))); y1 = min(ROWS - 1, int(math.ceil(F32(F32(F32(v - miny) + r) * hinv))))
    best, best_idx = None, -1
    if x0 >= COLS or x1 < 0 or y0 >= ROWS or y1 < 0:
        return -1, None
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for i in cells[ix][iy]:
                if not (abs(F32(keys["x"][i] - u)) < r and abs(F32(keys["y"][i] - v)) < r):
                    continue
                if keys["octave"][i] < level - 1 or keys["octave"][i] > level:
                    continue
                d = hamming(qdesc, desc[i])
                if best is None or d < best:
                    best, best_idx = d, i
    return best_idx, best


def search(scene, fma, thr, scale):
    kfs, cam, bounds = scene["keyframes"], scene["camera4"], scene["bounds4"]
    grids = {}
    out = []
    for p in scene["problems"]:
        sR12, sR21, t21 = similarity(p["s12"], p["R12"], p["t12"])
        t12 = np.asarray(p["t12"], F32)
        side = []
        for d, (src, tgt, sR, t, done) in enumerate(((p["kf1"], p["kf2"], sR21, t21, p.get("matched1")),
                                                     (p["kf2"], p["kf1"], sR12, t12, p.get("matched2")))):
            S, T = kfs[src], kfs[tgt]
            n = len(S["keys_un"])
            Tcw = np.asarray(S["Tcw"], F32).reshape(4, 4)
            if tgt not in grids:
                grids[tgt] = grid_of(T["keys_un"], bounds)
            st, best, lvl, uv = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros((n, 2), F32)
            for i in range(n):
                if not S["has_point"][i] or (done is not None and done[i]):
                    continue
                s, u, v, level, r = project(np.asarray(S["world_pos"][i], F32), Tcw[:3, :3], Tcw[:3, 3], sR, t, cam, bounds, p["th"],
                                            S["min_distance"][i], S["max_distance"][i], fma, thr, scale)
                st[i], uv[i], lvl[i] = s, (u, v), level
                if s != NO_CANDIDATE:
                    continue
                idx, dist = best_in_area(grids[tgt], T["keys_un"], T["desc"], u, v, r, level, S["point_desc"][i])
                if idx < 0:
                    continue
                if dist > TH_HIGH:
                    st[i] = TOO_FAR
                else:
                    st[i], best[i] = MATCH, idx
            side.append((st, best, lvl, uv))
        (st1, b1, l1, uv1), (st2, b2, l2, uv2) = side
        m = np.array([b1[i] if b1[i] >= 0 and b2[b1[i]] == i else -1 for i in range(len(b1))], np.int32).reshape(-1)
        out.append(dict(n=int((m >= 0).sum()), matches=m, status1=st1, status2=st2, best1=b1, best2=b2, level1=l1, level2=l2,
                        uv1=uv1, uv2=uv2))
    return out


def stage1(scene, fma, thr, scale, k):
    """the projected-point views the single orbx_search_by_sim3 / oracle.search_by_sim3 take for problem k"""
    res = search(scene, fma, thr, scale)[k]
    p = scene["problems"][k]
    views = []
    for which, src in ((1, p["kf1"]), (2, p["kf2"])):
        st, lvl, uv = res["status%d" % which], res["level%d" % which], res["uv%d" % which]
        valid = (st >= NO_CANDIDATE).astype(np.uint8)
        views.append(dict(valid=valid, uv=np.where(valid[:, None] > 0, uv, 0).astype(F32), level=np.where(valid > 0, lvl, 0).astype(np.int32),
                          desc=np.ascontiguousarray(scene["keyframes"][src]["point_desc"], np.uint8).reshape(-1, 32)))
    return views[0], views[1], res
