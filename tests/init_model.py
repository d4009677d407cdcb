"""The H / F RANSAC of Initializer (src/Initializer.cc) restated in numpy, independently of csrc/orbx_init.h: Normalize, ComputeH21,
ComputeF21, the de-normalisation, CheckHomography, CheckFundamental, the strict > best update, RH and the choice of model, with
what DESIGN.md section 2 (F14) fixes where the reference calls OpenCV.  Every step is a float32 scalar operation, written once
and applied to all hypotheses of a problem at a time (one array element per hypothesis): numpy's elementwise float32 + - * /
sqrt are the IEEE operations, nothing is fused and no sum is reordered.  A hypothesis whose Jacobi has finished is at a fixed
point (a sweep without a rotation repeats itself), so running the sweeps of all hypotheses in lockstep changes nothing."""
import numpy as np

F = np.float32
D = np.float64
NONE, H, FUND = 0, 1, 2
SWEEPS = 30
SVD_EPS = F(1e-12)
SVD_TINY = F(1e-12)
TH_H = F(5.991)
TH_F = F(3.841)
TH_SCORE = F(5.991)


def canon(a):
    a = np.array(a, F, copy=True)
    b = a.view(np.uint32)
    b[np.isnan(a)] = 0x7fc00000
    return a


def normalize(keys):
    """Normalize over ALL keypoints: T (3x3) and (meanX, meanY, sX, sY)"""
    keys = np.asarray(keys, F).reshape(-1, 2)
    N = len(keys)
    with np.errstate(all="ignore"):
        mx, my = F(0), F(0)
        for x, y in keys:
            mx = mx + x
            my = my + y
        mx = mx / F(N)
        my = my / F(N)
        dx, dy = F(0), F(0)
        for x, y in keys:
            dx = dx + np.abs(x - mx)
            dy = dy + np.abs(y - my)
        dx = dx / F(N)
        dy = dy / F(N)
        sx = F(1) / dx
        sy = F(1) / dy
        T = np.eye(3, dtype=F)
        T[0, 0], T[1, 1], T[0, 2], T[1, 2] = sx, sy, (-mx) * sx, (-my) * sy
    return T, (mx, my, sx, sy)


def jacobi(A):
    """one-sided Jacobi over the columns of A [B, m, nc]: the rotated A, V, and the column of smallest squared norm"""
    with np.errstate(all="ignore"):
        return _jacobi(A)


def _jacobi(A):
    A = np.array(A, F, copy=True)
    B, m, nc = A.shape
    V = np.zeros((B, nc, nc), F)
    V[:, np.arange(nc), np.arange(nc)] = 1
    for sweep in range(SWEEPS):
        rotated = False
        for p in range(nc - 1):
            for q in range(p + 1, nc):
                alpha, beta, gamma = np.zeros(B, F), np.zeros(B, F), np.zeros(B, F)
                for k in range(m):
                    ap, aq = A[:, k, p], A[:, k, q]
                    alpha = alpha + ap * ap
                    beta = beta + aq * aq
                    gamma = gamma + ap * aq
                rot = (gamma * gamma > SVD_EPS * (alpha * beta)) & (alpha > SVD_TINY * beta) & (beta > SVD_TINY * alpha)
                if not rot.any():
                    continue
                rotated = True
                zeta = (beta - alpha) / (F(2) * gamma)
                den = np.abs(zeta) + np.sqrt(zeta * zeta + F(1))
                t = np.where(zeta < 0, F(-1), F(1)) / den
                c = F(1) / np.sqrt(t * t + F(1))
                s = t * c
                for M in (A, V):
                    xp, xq = M[:, :, p].copy(), M[:, :, q].copy()
                    M[:, :, p] = np.where(rot[:, None], c[:, None] * xp - s[:, None] * xq, xp)
                    M[:, :, q] = np.where(rot[:, None], s[:, None] * xp + c[:, None] * xq, xq)
        if not rotated:
            break
    best = np.zeros(B, np.int64)
    least = None
    for j in range(nc):
        nj = np.zeros(B, F)
        for k in range(m):
            nj = nj + A[:, k, j] * A[:, k, j]
        if j == 0:
            least = nj
        else:
            upd = nj < least
            least = np.where(upd, nj, least)
            best = np.where(upd, j, best)
    return A, V, best


def build_A(pn, is_h):
    """pn [B, 8, 4]: the normalised u1 v1 u2 v2 of the eight drawn matches; A [B, 16, 9] or [B, 8, 9]"""
    B = len(pn)
    u1, v1, u2, v2 = (pn[:, :, c] for c in range(4))
    one, zero = np.ones_like(u1), np.zeros_like(u1)
    if is_h:
        A = np.zeros((B, 16, 9), F)
        A[:, 0::2] = np.stack([zero, zero, zero, -u1, -v1, -one, v2 * u1, v2 * v1, v2], axis=2)
        A[:, 1::2] = np.stack([u1, v1, one, zero, zero, zero, (-u2) * u1, (-u2) * v1, -u2], axis=2)
        return A
    return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, one], axis=2).astype(F)


def null_vector(A):
    """[B, 9]: the right singular vector of the smallest singular value, as the library fixes it"""
    _, V, col = jacobi(A)
    return V[np.arange(len(A)), :, col]


def mul3(a, b):
    """a b for [B, 3, 3] (or [3, 3]) float32: (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j"""
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    o = np.zeros(a.shape, F)
    for i in range(3):
        for j in range(3):
            o[..., i, j] = (a[..., i, 0] * b[..., 0, j] + a[..., i, 1] * b[..., 1, j]) + a[..., i, 2] * b[..., 2, j]
    return o


def inv3(m):
    """adjugate over the determinant in double, each entry rounded to float once"""
    m = np.asarray(m, F).astype(D)
    a, b, c, d, e, f, g, h, i = (m[..., r, s] for r in range(3) for s in range(3))
    k0, k1, k2 = e * i - f * h, d * i - f * g, d * h - e * g
    det = (a * k0 - b * k1) + c * k2
    r = 1.0 / det
    o = np.stack([k0 * r, (c * h - b * i) * r, (b * f - c * e) * r, (f * g - d * i) * r, (a * i - c * g) * r, (c * d - a * f) * r,
                  k2 * r, (b * g - a * h) * r, (a * e - b * d) * r], axis=-1)
    return o.astype(F).reshape(m.shape)


def hypotheses(pn, is_h, T1, T2):
    """M [B, 3, 3], Minv [B, 3, 3] (zeros for F), bad [B]"""
    x = null_vector(build_A(pn, is_h))
    B = len(x)
    if is_h:
        Mn = x.reshape(B, 3, 3)
        left = inv3(T2)
    else:
        G, GV, drop = jacobi(x.reshape(B, 3, 3))
        c0 = np.where(drop == 0, 1, 0)
        c1 = np.where(drop == 2, 1, 2)
        r = np.arange(B)
        Mn = np.zeros((B, 3, 3), F)
        for i in range(3):
            for j in range(3):
                Mn[:, i, j] = G[r, i, c0] * GV[r, j, c0] + G[r, i, c1] * GV[r, j, c1]
        left = T2.T
    M = mul3(mul3(left[None], Mn), T1[None])
    Minv = inv3(M) if is_h else np.zeros((B, 3, 3), F)
    bad = ~np.isfinite(M).all(axis=(1, 2)) | ~np.isfinite(Minv).all(axis=(1, 2))
    return canon(M), canon(Minv), bad


def check(M, Minv, is_h, raw, sigma):
    """scores [B] and masks [B, n] over the un-normalised matches raw [n, 4], in match order"""
    B = len(M)
    n = len(raw)
    inv_s2 = F(1) / (F(sigma) * F(sigma))
    score = np.zeros(B, F)
    mask = np.zeros((B, n), bool)
    m = [[M[:, i, j] for j in range(3)] for i in range(3)]
    w = [[Minv[:, i, j] for j in range(3)] for i in range(3)]
    for k in range(n):
        u1, v1, u2, v2 = (F(c) for c in raw[k])
        if is_h:
            wi = F(1) / ((w[2][0] * u2 + w[2][1] * v2) + w[2][2])
            a = ((w[0][0] * u2 + w[0][1] * v2) + w[0][2]) * wi
            b = ((w[1][0] * u2 + w[1][1] * v2) + w[1][2]) * wi
            chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_s2
            wi = F(1) / ((m[2][0] * u1 + m[2][1] * v1) + m[2][2])
            a = ((m[0][0] * u1 + m[0][1] * v1) + m[0][2]) * wi
            b = ((m[1][0] * u1 + m[1][1] * v1) + m[1][2]) * wi
            chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_s2
            th, ths = TH_H, TH_H
        else:
            a2 = (m[0][0] * u1 + m[0][1] * v1) + m[0][2]
            b2 = (m[1][0] * u1 + m[1][1] * v1) + m[1][2]
            c2 = (m[2][0] * u1 + m[2][1] * v1) + m[2][2]
            num2 = (a2 * u2 + b2 * v2) + c2
            chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * inv_s2
            a1 = (m[0][0] * u2 + m[1][0] * v2) + m[2][0]
            b1 = (m[0][1] * u2 + m[1][1] * v2) + m[2][1]
            c1 = (m[0][2] * u2 + m[1][2] * v2) + m[2][2]
            num1 = (a1 * u1 + b1 * v1) + c1
            chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * inv_s2
            th, ths = TH_F, TH_SCORE
        out1 = chi1 > th                                        # a NaN compares false: bIn stays, the NaN enters the score
        score = np.where(out1, score, score + (ths - chi1))
        out2 = chi2 > th
        score = np.where(out2, score, score + (ths - chi2))
        mask[:, k] = ~out1 & ~out2
    return canon(score), mask


def best_of(scores):
    score, it = F(0), -1
    for i, s in enumerate(scores):
        if s > score:
            score, it = s, i
    return score, it


def solve(p):
    """one problem (a dict as tests/init_scenes.py makes them) -> dict of everything the library reports"""
    with np.errstate(all="ignore"):
        keys1, keys2 = np.asarray(p["keys1"], F).reshape(-1, 2), np.asarray(p["keys2"], F).reshape(-1, 2)
        matches = np.asarray(p["matches"], np.int64).reshape(-1, 2)
        n, models = len(matches), int(p.get("models", H | FUND))
        T1, (mx1, my1, sx1, sy1) = normalize(keys1)
        T2, (mx2, my2, sx2, sy2) = normalize(keys2)
        out = dict(T1=canon(T1), T2=canon(T2), SH=F(0), SF=F(0), itH=-1, itF=-1, model=NONE, per={})
        if n >= 8 and models:
            a, b = keys1[matches[:, 0]], keys2[matches[:, 1]]
            pn = np.stack([(a[:, 0] - mx1) * sx1, (a[:, 1] - my1) * sy1, (b[:, 0] - mx2) * sx2, (b[:, 1] - my2) * sy2], axis=1).astype(F)
            raw = np.concatenate([a, b], axis=1)
            sets = np.asarray(p["sets"], np.int64).reshape(-1, 8)
            for model in (H, FUND):
                if models & model:
                    M, Minv, bad = hypotheses(pn[sets], model == H, T1, T2)
                    scores, masks = check(M, Minv, model == H, raw, p["sigma"])
                    out["per"][model] = dict(M=M, Minv=Minv, bad=bad, scores=scores, masks=masks)
                    s, it = best_of(scores)
                    if model == H:
                        out["SH"], out["itH"] = s, it
                    else:
                        out["SF"], out["itF"] = s, it
        out["RH"] = canon(out["SH"] / (out["SH"] + out["SF"]))[()]
        if out["itH"] >= 0 or out["itF"] >= 0:
            out["model"] = H if D(out["RH"]) > 0.40 else FUND
    return out
