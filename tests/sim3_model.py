"""Sim3Solver (src/Sim3Solver.cc) restated in numpy, independently of csrc/orbx_sim3.h: the constructor's projections
(FromCameraToImage, :550-569), SetRansacParameters (:153-191), ComputeSim3 (:329-454), Project (:517-541), CheckInliers (:460-490)
and the iterate state machine (:202-294), with numpy float32 / float64 scalars where the source has float / double.  What the
source leaves to OpenCV or libm is taken from DESIGN.md section 2 (F12): the cyclic Jacobi for cv::eigen, cv::norm, the MatExpr
scaling, cv::Rodrigues, the order of the 3x3 float products, cv::Mat::dot.  Exactly two primitives come from the library:
orbx_pose_sin_cos and orbx_sim3_atan2.

horn_float64 is a float64 comparator (Horn's closed form through numpy.linalg.eigh), used only for the accuracy check."""
import ctypes as C

import numpy as np

F = np.float32
D = np.float64
F0, F1, F2, F3 = F(0), F(1), F(2), F(3)
SWEEPS = 10
STOP = F(1e-14)                       # a sweep runs while off > STOP * dia
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
DBL_EPSILON = 2.0 ** -52


def _lib():
    from orb_slam2_detailed_comments_amd import _capi
    return _capi.lib()


def sincos(theta):
    s, c = C.c_double(), C.c_double()
    _lib().orbx_pose_sin_cos(float(theta), C.byref(s), C.byref(c))
    return D(s.value), D(c.value)


def atan2(y, x):
    return D(_lib().orbx_sim3_atan2(float(y), float(x)))


def ransac_iterations(n, probability=0.99, min_inliers=6, max_iterations=300):
    """SetRansacParameters: what mRansacMaxIts becomes"""
    with np.errstate(all="ignore"):
        epsilon = F(min_inliers) / F(n)
        if min_inliers == n:
            nit = 1
        else:
            v = np.ceil(np.log(D(1) - D(probability)) / np.log(D(1) - np.power(D(epsilon), D(3))))
            # outside int's range the source's conversion is undefined; F12: NaN and large values count as INT_MAX
            nit = 2 ** 31 - 1 if not (v < 2.0 ** 31) else -2 ** 31 if v < -2.0 ** 31 else int(v)
    return max(1, min(nit, max_iterations))


def to_image(X, K):
    """FromCameraToImage for points X [n, 3] float32; K = fx, fy, cx, cy.  Returns [n, 2] float32."""
    X = np.asarray(X, F).reshape(-1, 3)
    K = np.asarray(K, F)
    with np.errstate(all="ignore"):
        invz = F1 / X[:, 2]
        x = X[:, 0] * invz
        y = X[:, 1] * invz
        return np.stack([K[0] * x + K[2], K[1] * y + K[3]], axis=1)


def project(X, T, K):
    """Project: Rcw * X + tcw per row (k = 0, 1, 2 in order, then + t), then FromCameraToImage; T 4x4 float32"""
    X = np.asarray(X, F).reshape(-1, 3)
    T = np.asarray(T, F).reshape(4, 4)
    with np.errstate(all="ignore"):
        c = [((T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]) + T[r, 3] for r in range(3)]
    return to_image(np.stack(c, axis=1), K)


def _err(a, b):
    d = a - b                                                   # float32
    dx, dy = d[:, 0].astype(D), d[:, 1].astype(D)
    with np.errstate(all="ignore"):
        return (dx * dx + dy * dy).astype(F)                    # cv::Mat::dot in double, const float err


def check_inliers(H, prob):
    """CheckInliers: the mask (bool [n]) of hypothesis H"""
    p2im1 = project(prob["x2c"], H["T12"], prob["camera1"])
    p1im2 = project(prob["x1c"], H["T21"], prob["camera2"])
    err1 = _err(prob["p1im1"], p2im1)
    err2 = _err(p1im2, prob["p2im2"])
    with np.errstate(all="ignore"):
        return (err1 < prob["max_err1"]) & (err2 < prob["max_err2"])


def eigen4(N):
    """the library's cv::eigen of the symmetric 4x4 float matrix: cyclic Jacobi (F12); returns the eigenvector (4 float32) of
    the largest eigenvalue, first on a tie, and the number of sweeps that ran"""
    a = [[F(N[min(i, j)][max(i, j)]) for j in range(4)] for i in range(4)]
    v = [[F1 if i == j else F0 for j in range(4)] for i in range(4)]
    sweeps = 0
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            off = F0
            for k, (p, q) in enumerate(PAIRS):
                sq = a[p][q] * a[p][q]
                off = sq if k == 0 else off + sq
            dia = ((a[0][0] * a[0][0] + a[1][1] * a[1][1]) + a[2][2] * a[2][2]) + a[3][3] * a[3][3]
            if not (off > STOP * dia):
                break
            sweeps += 1
            for p, q in PAIRS:
                apq = a[p][q]
                if apq == F0:
                    continue
                theta = (a[q][q] - a[p][p]) / (F2 * apq)
                den = np.abs(theta) + np.sqrt(theta * theta + F1)
                t = (F(-1) if theta < F0 else F1) / den
                c = F1 / np.sqrt(t * t + F1)
                s = t * c
                h = t * apq
                a[p][p] = a[p][p] - h
                a[q][q] = a[q][q] + h
                a[p][q] = a[q][p] = F0
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = a[r][p], a[r][q]
                        a[r][p] = a[p][r] = c * arp - s * arq
                        a[r][q] = a[q][r] = s * arp + c * arq
                    vrp, vrq = v[r][p], v[r][q]
                    v[r][p] = c * vrp - s * vrq
                    v[r][q] = s * vrp + c * vrq
        best, col = a[0][0], 0
        for k in range(1, 4):
            if a[k][k] > best:
                best, col = a[k][k], k
    return [v[r][col] for r in range(4)], sweeps


def rodrigues(r):
    """the library's cv::Rodrigues (F12): double, rounded to float32; r = 3 float32"""
    with np.errstate(all="ignore"):
        rx, ry, rz = D(r[0]), D(r[1]), D(r[2])
        theta = np.sqrt((rx * rx + ry * ry) + rz * rz)
        if theta < DBL_EPSILON:
            return np.eye(3, dtype=F)
        sn, cs = sincos(theta)
        u = (rx / theta, ry / theta, rz / theta)
        c1 = D(1) - cs
        Z = D(0)
        K = ((Z, -u[2], u[1]), (u[2], Z, -u[0]), (-u[1], u[0], Z))
        R = np.empty((3, 3), F)
        for i in range(3):
            for j in range(3):
                R[i, j] = F(((cs if i == j else Z) + (c1 * u[i]) * u[j]) + sn * K[i][j])
    return R


def _mat3(A, B):
    """3x3 float product, k = 0, 1, 2 in order, every product and sum rounded to float32"""
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def compute_sim3(X1, X2, fix_scale, trace=None):
    """ComputeSim3 for the three correspondences X1, X2 [3 points, 3] float32 (the columns of the source's P1, P2)"""
    X1 = np.asarray(X1, F).reshape(3, 3)
    X2 = np.asarray(X2, F).reshape(3, 3)
    with np.errstate(all="ignore"):
        O1 = [((X1[0, r] + X1[1, r]) + X1[2, r]) / F3 for r in range(3)]
        O2 = [((X2[0, r] + X2[1, r]) + X2[2, r]) / F3 for r in range(3)]
        Pr1 = [[X1[c, r] - O1[r] for c in range(3)] for r in range(3)]      # [row][col]
        Pr2 = [[X2[c, r] - O2[r] for c in range(3)] for r in range(3)]
        Pr1t = [[Pr1[j][i] for j in range(3)] for i in range(3)]
        M = _mat3(Pr2, Pr1t)
        m = [[D(M[i][j]) for j in range(3)] for i in range(3)]
        N11 = F((m[0][0] + m[1][1]) + m[2][2]); N12 = F(m[1][2] - m[2][1]); N13 = F(m[2][0] - m[0][2]); N14 = F(m[0][1] - m[1][0])
        N22 = F((m[0][0] - m[1][1]) - m[2][2]); N23 = F(m[0][1] + m[1][0]); N24 = F(m[2][0] + m[0][2])
        N33 = F((-m[0][0] + m[1][1]) - m[2][2]); N34 = F(m[1][2] + m[2][1]); N44 = F((-m[0][0] - m[1][1]) + m[2][2])
        N = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
        q, sweeps = eigen4(N)
        v = [D(q[1]), D(q[2]), D(q[3])]
        nv = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        ang = atan2(nv, D(q[0]))
        f = (D(2) * ang) / nv
        rv = [F(f * v[0]), F(f * v[1]), F(f * v[2])]
        R = rodrigues(rv)
        P3 = _mat3(R, Pr2)
        if fix_scale:
            s = F1
        else:
            nom = den = D(0)
            for i in range(3):
                for j in range(3):
                    nom = nom + D(Pr1[i][j]) * D(P3[i][j])
                    den = den + D(P3[i][j] * P3[i][j])
            s = F(nom / den)
        inv = D(1) / D(s)
        sR = [[s * R[i, j] for j in range(3)] for i in range(3)]
        sRi = [[F(inv * D(R[j, i])) for j in range(3)] for i in range(3)]
        t = [O1[i] - ((sR[i][0] * O2[0] + sR[i][1] * O2[1]) + sR[i][2] * O2[2]) for i in range(3)]
        T12 = np.eye(4, dtype=F)
        T21 = np.eye(4, dtype=F)
        for i in range(3):
            for j in range(3):
                T12[i, j] = sR[i][j]
                T21[i, j] = sRi[i][j]
            T12[i, 3] = t[i]
            T21[i, 3] = -((sRi[i][0] * t[0] + sRi[i][1] * t[1]) + sRi[i][2] * t[2])
    if trace is not None:
        trace.update(sweeps=sweeps, q=q, ang=ang, nv=nv)
    return dict(T12=T12, T21=T21, R=R, t=np.array(t, F), s=F(s))


def hyp48(H):
    """a hypothesis as the library stores it: T12 | T21 | R | t | s | 3 x 0"""
    h = np.concatenate([H["T12"].ravel(), H["T21"].ravel(), H["R"].ravel(), H["t"], [H["s"]], np.zeros(3, F)]).astype(F)
    b = h.view(np.uint32)
    b[np.isnan(h)] = 0x7fc00000                                 # F12: a stored NaN is this one, whatever the processor made
    return h


def prepare(prob):
    """the constructor's part after the filters: mvP1im1, mvP2im2"""
    p = dict(prob)
    for k in ("x1c", "x2c"):
        p[k] = np.asarray(prob[k], F).reshape(-1, 3)
    for k in ("max_err1", "max_err2", "camera1", "camera2"):
        p[k] = np.asarray(prob[k], F)
    p["p1im1"] = to_image(p["x1c"], p["camera1"])
    p["p2im2"] = to_image(p["x2c"], p["camera2"])
    return p


def evaluate(prob):
    """every iteration of one problem: (hyps [it, 48] float32, masks [it, n] bool, counts [it] int32); None where the solver
    computes nothing (n < min_inliers)"""
    p = prepare(prob)
    n = len(p["x1c"])
    if n < p["min_inliers"]:
        return None
    sets = np.asarray(p["sets"], np.int64).reshape(-1, 3)
    assert len(sets) == p["iterations"]
    hyps, masks = [], []
    for s in sets:
        H = compute_sim3(p["x1c"][s], p["x2c"][s], p["fix_scale"])
        hyps.append(hyp48(H))
        masks.append(check_inliers(H, p))
    masks = np.array(masks, bool).reshape(len(sets), n)
    return np.array(hyps, F), masks, masks.sum(axis=1).astype(np.int32)


class Solver:
    """the iterate state machine over the evaluated iterations"""

    def __init__(self, prob, evaluated=None):
        self.n = len(np.asarray(prob["x1c"]).reshape(-1, 3))
        self.min_inliers = int(prob["min_inliers"])
        self.max_its = int(prob["iterations"])
        self.ev = evaluated if evaluated is not None or self.n < self.min_inliers else evaluate(prob)
        self.done = 0                  # mnIterations
        self.best_inliers = 0          # mnBestInliers
        self.best_it = -1

    def iterate(self, n_iterations):
        """returns (T12 4x4 or None, no_more, inliers bool [n], ninliers)"""
        inl = np.zeros(self.n, bool)
        if self.n < self.min_inliers:
            return None, True, inl, 0
        hyps, masks, counts = self.ev
        cur = 0
        while self.done < self.max_its and cur < n_iterations:
            cur += 1
            i = self.done
            self.done += 1
            if counts[i] >= self.best_inliers:
                self.best_inliers = int(counts[i])
                self.best_it = i
                if counts[i] > self.min_inliers:
                    return hyps[i][:16].reshape(4, 4).copy(), False, masks[i].copy(), int(counts[i])
        return None, self.done >= self.max_its, inl, 0

    def best(self):
        """(R 3x3, t 3, s) of the best hypothesis so far, or None before the first iteration"""
        if self.best_it < 0:
            return None
        h = self.ev[0][self.best_it]
        return h[32:41].reshape(3, 3).copy(), h[41:44].copy(), h[44]


def horn_float64(X1, X2):
    """Horn 1987 in float64 with numpy.linalg.eigh: the rotation that takes the centred X2 to the centred X1"""
    A = np.asarray(X1, D).reshape(3, 3).T
    B = np.asarray(X2, D).reshape(3, 3).T
    Pr1 = A - A.mean(axis=1, keepdims=True)
    Pr2 = B - B.mean(axis=1, keepdims=True)
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, V = np.linalg.eigh(N)
    q0, q1, q2, q3 = V[:, np.argmax(w)]
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])
