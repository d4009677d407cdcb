"""ReconstructF, ReconstructH, DecomposeE, CheckRT and Triangulate of Initializer (src/Initializer.cc) restated in numpy,
independently of csrc/orbx_recon.h, with what DESIGN.md section 2 (F15) fixes where the reference calls OpenCV or libm.  Every
step is a float32 (or, where F15 says so, float64) scalar operation; CheckRT is written once and applied to all inlier matches
of a hypothesis at a time (one array element per match): numpy's elementwise + - * / sqrt are the IEEE operations, nothing is
fused and no sum is reordered.  The one-sided Jacobi is tests/init_model.py's (F14 fixed it); acosf is the C library's, called
through ctypes, as the library's host side calls it."""
import ctypes
import ctypes.util

import numpy as np

import init_model as im

F = np.float32
D = np.float64
H, FUND = im.H, im.FUND
IDX = 50
CV_PI = 3.1415926535897932384626433832795

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.acosf.restype = ctypes.c_float
_libm.acosf.argtypes = [ctypes.c_float]


def canon(a):
    return im.canon(a)


def det3(m):
    """float64: (a k0 - b k1) + c k2"""
    a, b, c, d, e, f, g, h, i = (D(v) for v in np.asarray(m, F).reshape(9))
    k0, k1, k2 = e * i - f * h, d * i - f * g, d * h - e * g
    return (a * k0 - b * k1) + c * k2


def norm3(x, y, z):
    """cv::norm: squares summed in float64 in index order, sqrt; works on scalars and arrays"""
    a, b, c = np.asarray(x, F).astype(D), np.asarray(y, F).astype(D), np.asarray(z, F).astype(D)
    return np.sqrt((a * a + b * b) + c * c)


def div(x, s):
    """Mat / scalar: float64 division, rounded to float32 once"""
    return (np.asarray(x, F).astype(D) / D(s)).astype(F)


def mulv(m, x, y, z):
    m = np.asarray(m, F)
    return [(m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z for i in range(3)]


def svd3(M):
    """U, w, Vt of a 3 x 3 float32 matrix as F15 fixes them"""
    A, V, _ = im.jacobi(np.asarray(M, F).reshape(1, 3, 3))
    A, V = A[0], V[0]
    n = [F(0), F(0), F(0)]
    for k in range(3):
        for j in range(3):
            n[j] = n[j] + A[k, j] * A[k, j]
    idx = [0, 1, 2]
    for a, b in ((0, 1), (1, 2), (0, 1)):
        if n[b] > n[a]:
            n[a], n[b] = n[b], n[a]
            idx[a], idx[b] = idx[b], idx[a]
    w = np.array([np.sqrt(n[0]), np.sqrt(n[1]), np.sqrt(n[2])], F)
    U = np.zeros((3, 3), F)
    U[:, 0] = A[:, idx[0]] / w[0]
    U[:, 1] = A[:, idx[1]] / w[1]
    c2 = A[:, idx[2]]
    x = U[1, 0] * U[2, 1] - U[2, 0] * U[1, 1]
    y = U[2, 0] * U[0, 1] - U[0, 0] * U[2, 1]
    z = U[0, 0] * U[1, 1] - U[1, 0] * U[0, 1]
    d = (x * c2[0] + y * c2[1]) + z * c2[2]
    if d < 0:
        x, y, z = -x, -y, -z
    U[:, 2] = (x, y, z)
    Vt = np.stack([V[:, idx[0]], V[:, idx[1]], V[:, idx[2]]]).astype(F)
    return U, w, Vt


def K9(K4):
    fx, fy, cx, cy = (F(v) for v in K4)
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)


def pose(K, R, t, n=None):
    """the record of one hypothesis: R, t, n, P2 = K [R | t], O2 = -R^T t"""
    R, t = np.asarray(R, F), np.asarray(t, F)
    X = np.concatenate([R, t.reshape(3, 1)], axis=1)
    P2 = np.zeros((3, 4), F)
    for i in range(3):
        for j in range(4):
            P2[i, j] = (K[i, 0] * X[0, j] + K[i, 1] * X[1, j]) + K[i, 2] * X[2, j]
    O2 = np.array([((-R[0, i]) * t[0] + (-R[1, i]) * t[1]) + (-R[2, i]) * t[2] for i in range(3)], F)
    return dict(R=canon(R), t=canon(t), n=canon(np.zeros(3, F) if n is None else n), P2=canon(P2), O2=canon(O2), valid=True)


def decompose_f(F21, K4):
    K = K9(K4)
    E = im.mul3(im.mul3(K.T.copy(), np.asarray(F21, F)), K)
    U, w, Vt = svd3(E)
    t = div(U[:, 2], norm3(U[0, 2], U[1, 2], U[2, 2]))
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)
    R1 = im.mul3(im.mul3(U, W), Vt)
    if det3(R1) < 0:
        R1 = -R1
    R2 = im.mul3(im.mul3(U, W.T.copy()), Vt)
    if det3(R2) < 0:
        R2 = -R2
    return [pose(K, R1, t), pose(K, R2, t), pose(K, R1, -t), pose(K, R2, -t)], dict(U=U, w=w, Vt=Vt, M=E)


def decompose_h(H21, K4):
    """the eight poses, or None where the source returns false before any hypothesis"""
    K = K9(K4)
    A = im.mul3(im.mul3(im.inv3(K), np.asarray(H21, F)), K)
    U, w, Vt = svd3(A)
    info = dict(U=U, w=w, Vt=Vt, M=A)
    s = F(det3(U) * det3(Vt))
    d1, d2, d3 = w
    if D(d1 / d2) < 1.00001 or D(d2 / d3) < 1.00001:
        return None, info
    aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1 = [aux1, aux1, -aux1, -aux1]
    x3 = [aux3, -aux3, aux3, -aux3]
    aux_stheta = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    stheta = [aux_stheta, -aux_stheta, -aux_stheta, aux_stheta]
    aux_sphi = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sphi = [aux_sphi, -aux_sphi, -aux_sphi, aux_sphi]
    V = Vt.T.copy()
    out = []
    for second in (False, True):
        for i in range(4):
            Rp = np.eye(3, dtype=F)
            if not second:
                Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ctheta, -stheta[i], stheta[i], ctheta
                tp = [x1[i] * (d1 - d3), F(0) * (d1 - d3), (-x3[i]) * (d1 - d3)]
            else:
                Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cphi, sphi[i], F(-1), sphi[i], -cphi
                tp = [x1[i] * (d1 + d3), F(0) * (d1 + d3), x3[i] * (d1 + d3)]
            R = s * im.mul3(im.mul3(U, Rp), Vt)
            t = np.array(mulv(U, *tp), F)
            t = div(t, norm3(*t))
            n = np.array(mulv(V, x1[i], F(0), x3[i]), F)
            if n[2] < 0:
                n = -n
            out.append(pose(K, R, t, n))
    return out, info


def key(c):
    """the monotone integer key of a float32: the order the cosine is selected by"""
    b = np.ascontiguousarray(c, F).view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, (~b) & 0xffffffff, b | 0x80000000)


def check_rt(P, K4, sigma, u1, v1, u2, v2):
    """CheckRT over the inlier matches given as float32 arrays: status (1, 2, 3 or 0), points [m, 3], cosines [m]"""
    fx, fy, cx, cy = (F(v) for v in K4)
    K = K9(K4)
    th2 = F(4.0 * D(F(sigma) * F(sigma)))
    m = len(u1)
    P1 = np.concatenate([K, np.zeros((3, 1), F)], axis=1)
    P2 = P["P2"]
    A = np.zeros((m, 4, 4), F)
    for j in range(4):
        A[:, 0, j] = u1 * P1[2, j] - P1[0, j]
        A[:, 1, j] = v1 * P1[2, j] - P1[1, j]
        A[:, 2, j] = u2 * P2[2, j] - P2[0, j]
        A[:, 3, j] = v2 * P2[2, j] - P2[1, j]
    _, V, col = im.jacobi(A)
    x = V[np.arange(m), :, col]
    X, Y, Z = x[:, 0] / x[:, 3], x[:, 1] / x[:, 3], x[:, 2] / x[:, 3]
    finite = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
    a0, a1, a2 = X - F(0), Y - F(0), Z - F(0)
    dist1 = norm3(a0, a1, a2).astype(F)
    b0, b1, b2 = X - P["O2"][0], Y - P["O2"][1], Z - P["O2"][2]
    dist2 = norm3(b0, b1, b2).astype(F)
    dot = (a0.astype(D) * b0.astype(D) + a1.astype(D) * b1.astype(D)) + a2.astype(D) * b2.astype(D)
    cosp = (dot / (dist1 * dist2).astype(D)).astype(F)
    low = cosp.astype(D) < 0.99998
    rej = (Z <= 0) & low
    R, t = P["R"], P["t"]
    p2 = mulv(R, X, Y, Z)
    p2 = [p2[0] + t[0], p2[1] + t[1], p2[2] + t[2]]
    rej |= (p2[2] <= 0) & low
    invZ1 = F(1) / Z
    im1x, im1y = fx * X * invZ1 + cx, fy * Y * invZ1 + cy
    rej |= ((im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1)) > th2
    invZ2 = F(1) / p2[2]
    im2x, im2y = fx * p2[0] * invZ2 + cx, fy * p2[1] * invZ2 + cy
    rej |= ((im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2)) > th2
    status = np.where(~finite, 1, np.where(rej, 0, np.where(low, 3, 2))).astype(np.uint8)
    counted = status >= 2
    pts = np.where(counted[:, None], np.stack([X, Y, Z], axis=1), F(0)).astype(F)
    return status, pts, canon(np.where(counted, cosp, F(0)))


def parallax_of(nGood, cosine):
    if nGood <= 0:
        return F(0)
    a = F(_libm.acosf(float(cosine))) * F(180)
    return canon(F(D(a) / D(CV_PI)))[()]


def solve(p):
    """one problem (a dict as tests/recon_scenes.py makes them) -> dict of everything the library reports"""
    with np.errstate(all="ignore"):
        keys1, keys2 = np.asarray(p["keys1"], F).reshape(-1, 2), np.asarray(p["keys2"], F).reshape(-1, 2)
        matches = np.asarray(p["matches"], np.int64).reshape(-1, 2)
        inl = np.asarray(p["inliers"], bool).reshape(-1)
        n, N = len(matches), int(inl.sum())
        is_h = p["model"] == H
        nhyp = 8 if is_h else 4
        min_par, min_tri = F(p.get("min_parallax", 1.0)), int(p.get("min_triangulated", 50))
        zero = dict(R=np.zeros((3, 3), F), t=np.zeros(3, F), n=np.zeros(3, F), nGood=0, cosine=F(0), parallax=F(0), valid=False)
        out = dict(ok=False, R21=np.zeros((3, 3), F), t21=np.zeros(3, F), chosen=-1, status=np.zeros(n, np.uint8),
                   points=np.zeros((n, 3), F), N=N, hyp=[dict(zero) for _ in range(nhyp)], svd=None)
        if N == 0:
            return out
        poses, out["svd"] = decompose_h(p["M"], p["K"]) if is_h else decompose_f(p["M"], p["K"])
        if poses is None:
            return out
        a, b = keys1[matches[inl, 0]], keys2[matches[inl, 1]]
        per = []
        for i, P in enumerate(poses):
            st, pts, cos = check_rt(P, p["K"], p["sigma"], a[:, 0], a[:, 1], b[:, 0], b[:, 1])
            nGood = int((st >= 2).sum())
            cosine = F(0)
            if nGood > 0:
                c = cos[st >= 2]
                cosine = c[np.argsort(key(c), kind="stable")][min(IDX, nGood - 1)]
            full_st, full_pts = np.zeros(n, np.uint8), np.zeros((n, 3), F)
            full_st[inl], full_pts[inl] = st, pts
            per.append((full_st, full_pts))
            out["hyp"][i] = dict(R=P["R"], t=P["t"], n=P["n"], nGood=nGood, cosine=cosine, parallax=parallax_of(nGood, cosine), valid=True)
        good = [h["nGood"] for h in out["hyp"]]
        par = [h["parallax"] for h in out["hyp"]]
        if is_h:
            best, second, idx, best_par = 0, 0, -1, F(-1)
            for i in range(8):
                if good[i] > best:
                    second, best, idx, best_par = best, good[i], i, par[i]
                elif good[i] > second:
                    second = good[i]
            out["chosen"] = idx
            out["ok"] = bool(second < 0.75 * best and best_par >= min_par and best > min_tri and best > 0.9 * N)
        else:
            mx = max(good)
            n_min = max(int(0.9 * N), min_tri)
            similar = sum(1 for g in good if g > 0.7 * mx)
            out["chosen"] = good.index(mx)
            if not (mx < n_min or similar > 1):
                out["ok"] = bool(par[out["chosen"]] > min_par)
        if out["chosen"] >= 0:
            out["status"], out["points"] = per[out["chosen"]]
        if out["ok"]:
            out["R21"], out["t21"] = out["hyp"][out["chosen"]]["R"], out["hyp"][out["chosen"]]["t"]
    return out
