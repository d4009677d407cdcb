"""numpy restatement of MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:424-516) and MapPoint::UpdateNormalAndDepth
(:570-638) over a ragged batch, for tests/test_mappoint_batch_{cpu,gpu}.py and tests/test_compat_mappoint.py.  The medians come
from np.sort, not from the kernels' bisection; the float / double steps of the second function are those of the cv::Mat stand-in
(tests/compat_runtime/opencv2/core/core.hpp), one numpy scalar operation per rounding."""
import hashlib

import numpy as np

f32, f64 = np.float32, np.float64
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distance_matrix(rows):
    rows = np.asarray(rows, np.uint8).reshape(-1, 32)
    return _POP[rows[:, None, :] ^ rows[None, :, :]].sum(axis=2).astype(np.int32)


def distinct_one(rows):
    """(best_idx, best_median, medians) of one point; rows [N, 32] in the map's iteration order, bad keyframes left out"""
    rows = np.asarray(rows, np.uint8).reshape(-1, 32)
    n = len(rows)
    if n == 0:
        return -1, -1, np.zeros(0, np.int32)
    med = np.sort(distance_matrix(rows), axis=1)[:, (n - 1) // 2]
    best, best_median = 0, np.iinfo(np.int32).max
    for i in range(n):                                               # `if (median < BestMedian)`: the first of equal medians
        if med[i] < best_median:
            best, best_median = i, int(med[i])
    return best, best_median, med


def distinct_batch(obs_begin, desc, best_desc=None):
    """(best_idx, best_median, best_desc); rows without observations keep their row of best_desc (zeros when none is passed)"""
    obs_begin = np.asarray(obs_begin, np.int64)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    npts = len(obs_begin) - 1
    idx, med = np.full(npts, -1, np.int32), np.full(npts, -1, np.int32)
    out = np.zeros((npts, 32), np.uint8) if best_desc is None else np.array(best_desc, np.uint8).reshape(npts, 32).copy()
    for p in range(npts):
        rows = desc[obs_begin[p]:obs_begin[p + 1]]
        if len(rows):
            idx[p], med[p], _ = distinct_one(rows)
            out[p] = rows[idx[p]]
    return idx, med, out


def desc_hash(best_desc):
    return hashlib.sha256(np.ascontiguousarray(best_desc, np.uint8).tobytes()).hexdigest()


def scale_factors(levels=8, factor=1.2):
    """mvScaleFactors as ORBextractor builds them: float products of the float factor"""
    sf = np.ones(levels, f32)
    for l in range(1, levels):
        sf[l] = f32(sf[l - 1] * f32(factor))
    return sf


def _norm(d):
    s = f64(0.0)
    for c in range(3):                                               # Mat::dot: a double sum in element order
        s = s + f64(d[c]) * f64(d[c])
    return np.sqrt(s)


def normal_depth_one(pos, centers, ref_center, level_scale, last_scale):
    """(normal[3], min_distance, max_distance) of one point with len(centers) >= 1 observations, all float32"""
    pos = np.asarray(pos, f32)
    normal = np.zeros(3, f32)
    n = 0
    with np.errstate(all="ignore"):
        for c in np.asarray(centers, f32).reshape(-1, 3):
            d = (pos - c).astype(f32)                                # a - b: element-wise in float
            nrm = _norm(d)
            term = np.array([f32(f64(d[k]) / nrm) for k in range(3)], f32)   # a / s: in double, rounded once
            normal = (normal + term).astype(f32)                     # a + b: element-wise in float, in observation order
            n += 1
        pc = (pos - np.asarray(ref_center, f32)).astype(f32)
        dist = f32(_norm(pc))
        maxd = f32(dist * f32(level_scale))
        mind = f32(maxd / f32(last_scale))
        out = np.array([f32(f64(normal[k]) / f64(n)) for k in range(3)], f32)
    return out, mind, maxd


def normal_depth_batch(obs_begin, pos, centers, ref_center, ref_level, scale, normal=None, min_distance=None, max_distance=None):
    obs_begin = np.asarray(obs_begin, np.int64)
    npts = len(obs_begin) - 1
    pos, centers, ref_center = (np.asarray(x, f32).reshape(-1, 3) for x in (pos, centers, ref_center))
    nrm = np.zeros((npts, 3), f32) if normal is None else np.array(normal, f32).reshape(npts, 3).copy()
    mind = np.zeros(npts, f32) if min_distance is None else np.array(min_distance, f32).copy()
    maxd = np.zeros(npts, f32) if max_distance is None else np.array(max_distance, f32).copy()
    for p in range(npts):
        if obs_begin[p + 1] > obs_begin[p]:
            nrm[p], mind[p], maxd[p] = normal_depth_one(pos[p], centers[obs_begin[p]:obs_begin[p + 1]], ref_center[p],
                                                        scale[ref_level[p]], scale[len(scale) - 1])
    return nrm, mind, maxd


# ------------------------------------------------------------------------------------------------ scenes shared by the tests
SIZES = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130)


def flip(rng, d, nbits):
    d = np.array(d, np.uint8).copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def prototype_rows(rng, n, nproto=3, max_flips=6):
    """n descriptors drawn as a few prototypes with 0 .. max_flips flipped bits: medians tie, rows repeat"""
    protos = rng.integers(0, 256, (nproto, 32), dtype=np.uint8)
    return np.stack([flip(rng, protos[rng.integers(0, nproto)], int(rng.integers(0, max_flips + 1))) for _ in range(n)])


def tie_rows(rng, n):
    """n >= 4 rows in which two DIFFERENT rows share the smallest median: A = base ^ bit a, B = base ^ bit b, every other row
    base with f bits of its own flipped (disjoint from everyone else's).  d(A, C) = d(B, C) = 1 + f and d(A, B) = 2, so rows A
    and B hold the same distances; d(C, C') = 2 f >= 1 + f, so no other row has a smaller median.  A sits at n // 3, B last."""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    f = 1 if n - 2 > 100 else 2
    bits = rng.permutation(256)

    def with_bits(b):
        d = base.copy()
        for x in b:
            d[x >> 3] ^= np.uint8(1 << (x & 7))
        return d
    others = [with_bits(bits[2 + f * k:2 + f * (k + 1)]) for k in range(n - 2)]
    rows = others[:n // 3] + [with_bits(bits[:1])] + others[n // 3:] + [with_bits(bits[1:2])]
    return np.stack(rows)


def scene(seed=7, sizes=SIZES, repeats=3):
    """one ragged batch: every size `repeats` times with prototype rows, then for every size above 3 one point with duplicated
    rows and one with a planted tie (tie_rows), and points without rows at the front, in the middle and at the end.  Returns
    obs_begin [P + 1], desc [rows, 32]."""
    rng = np.random.default_rng(seed)
    pts = [np.zeros((0, 32), np.uint8)]
    for r in range(repeats):
        for n in sizes:
            pts.append(prototype_rows(rng, n, nproto=2 + r))
        if r == 0:
            pts.append(np.zeros((0, 32), np.uint8))
    for n in sizes:
        if n > 3:
            rows = prototype_rows(rng, n)
            rows[n // 2] = rows[0]                                   # duplicate descriptor rows
            rows[n - 1] = rows[1]
            pts.append(rows)
            pts.append(tie_rows(rng, n))
    pts.append(np.zeros((0, 32), np.uint8))
    obs_begin = np.concatenate([[0], np.cumsum([len(x) for x in pts])]).astype(np.int32)
    return obs_begin, np.concatenate(pts)


def young_mix(rng, npoints):
    return rng.integers(2, 9, npoints).astype(np.int32)


def mature_mix(rng, npoints):
    """most points 5-30 observations, about one in a hundred 100-300"""
    n = rng.integers(5, 31, npoints).astype(np.int32)
    big = rng.uniform(size=npoints) < 0.01
    n[big] = rng.integers(100, 301, int(big.sum()))
    return n
