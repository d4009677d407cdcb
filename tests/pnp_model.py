"""numpy restatement of PnPsolver (src/PnPsolver.cc) as csrc/orbx_pnp.h fixes it: one function per
source function, every expression operation by operation in the header's order, float64 / float32 as the source's types.

Two evaluation modes.  OWN: the primitives the reference leaves to OpenCV 1.x are this library's (cyclic Jacobi, the adjugate
inverse, qr_solve as the least-squares routine, one-sided Jacobi) -- the device, the host path and this mode agree bit for bit.
LAPACK: the same primitives go through numpy.linalg (eigh, inv, lstsq, svd) -- the stand-in for an OpenCV build, which cannot be
run here; it measures how far the library's choices are from another correct implementation and pins nothing bit for bit."""
from __future__ import annotations

import numpy as np

D = np.float64
F = np.float32
SWEEPS = 30
JACOBI_EPS = D(1e-40)
SVD_EPS = D(1e-30)
RANK_EPS = D(1e-9)
MASK64 = (1 << 64) - 1


class Lcg:
    """the stand-in DUtils::Random of tests/compat_pnp (and tests/compat_sim3)"""

    def __init__(self, seed):
        self.s = seed

    def randint(self, lo, hi):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & MASK64
        return lo + (self.s >> 33) % (hi - lo + 1)

    def draw(self, n, iterations, k=4):
        """the draws of iterate() (:293-310): k indices by swap-remove from the list of all indices, per iteration"""
        out = np.zeros((iterations, k), np.int32)
        for i in range(iterations):
            avail = list(range(n))
            for c in range(k):
                r = self.randint(0, len(avail) - 1)
                out[i, c] = avail[r]
                avail[r] = avail[-1]
                avail.pop()
        return out


# ------------------------------------------------------------------------------------------------ SetRansacParameters
def _to_int(v):
    return 2 ** 31 - 1 if not (v < 2.0 ** 31) else -2 ** 31 if v < -2.0 ** 31 else int(v)


def set_ransac_parameters(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """(:190-239) -> (mRansacMinInliers, mRansacMaxIts)"""
    with np.errstate(all="ignore"):
        eps = F(epsilon)
        nmin = _to_int(D(F(n) * eps))
        nmin = max(nmin, min_inliers, min_set)
        if eps < F(nmin) / F(n):
            eps = F(nmin) / F(n)
        if nmin == n:
            nit = 1
        else:
            nit = _to_int(np.ceil(np.log(D(1) - D(probability)) / np.log(D(1) - np.power(D(eps), D(3)))))
    return nmin, max(1, min(nit, max_iterations))


def max_error(sigma2, th2=5.991):
    """mvMaxError[i] = mvSigma2[i] * th2: float times float"""
    return (np.asarray(sigma2, F) * F(th2)).astype(F)


# ------------------------------------------------------------------------------------------------ the OpenCV-owned primitives
def jacobi_eig(a):
    """cvSVD(CV_SVD_U_T) of a symmetric matrix as F13 fixes it: (eigenvalues descending, V with the vectors as columns)"""
    a = np.array(a, D)
    d = a.shape[0]
    V = np.eye(d, dtype=D)
    for _ in range(SWEEPS):
        off = D(0)
        dia = D(0)
        for p in range(d):
            dia = dia + a[p, p] * a[p, p]
            for q in range(p + 1, d):
                off = off + a[p, q] * a[p, q]
        if not (off > JACOBI_EPS * dia):
            break
        for p in range(d - 1):
            for q in range(p + 1, d):
                apq = a[p, q]
                if apq != 0.0:
                    app, aqq = a[p, p], a[q, q]
                    theta = (aqq - app) / (D(2) * apq)
                    den = np.abs(theta) + np.sqrt(theta * theta + D(1))
                    t = (D(-1) if theta < 0.0 else D(1)) / den
                    c = D(1) / np.sqrt(t * t + D(1))
                    s = t * c
                    h = t * apq
                    cp, cq = a[:, p].copy(), a[:, q].copy()
                    n_p, n_q = c * cp - s * cq, s * cp + c * cq
                    a[:, p] = n_p
                    a[p, :] = n_p
                    a[:, q] = n_q
                    a[q, :] = n_q
                    a[p, p] = app - h
                    a[q, q] = aqq + h
                    a[p, q] = 0.0
                    a[q, p] = 0.0
                    vp, vq = V[:, p].copy(), V[:, q].copy()
                    V[:, p] = c * vp - s * vq
                    V[:, q] = s * vp + c * vq
    w = np.diag(a).copy()
    for i in range(d - 1):
        m = i
        for j in range(i + 1, d):
            if w[j] > w[m]:
                m = j
        if m != i:
            w[[i, m]] = w[[m, i]]
            V[:, [i, m]] = V[:, [m, i]]
    return w, V


def adjugate_inverse(c):
    """cvInvert(CC, CV_SVD) as F13 fixes it"""
    (c00, c01, c02), (c10, c11, c12), (c20, c21, c22) = c
    k00 = c11 * c22 - c12 * c21
    k01 = c10 * c22 - c12 * c20
    k02 = c10 * c21 - c11 * c20
    det = (c00 * k00 - c01 * k01) + c02 * k02
    return np.array([[k00 / det, (c02 * c21 - c01 * c22) / det, (c01 * c12 - c02 * c11) / det],
                     [(c12 * c20 - c10 * c22) / det, (c00 * c22 - c02 * c20) / det, (c02 * c10 - c00 * c12) / det],
                     [k02 / det, (c01 * c20 - c00 * c21) / det, (c00 * c11 - c01 * c10) / det]], D)


def qr_solve(A, b):
    """(:1380-1514) operation by operation, eta over rows k .. nr - 2 as the source reads them; singular branch: X = 0"""
    A = np.array(A, D)
    b = np.array(b, D)
    nr, nc = A.shape
    A1 = np.zeros(nc, D)
    A2 = np.zeros(nc, D)
    for k in range(nc):
        eta = np.abs(A[k, k])
        for i in range(k + 1, nr):
            elt = np.abs(A[i - 1, k])
            if eta < elt:
                eta = elt
        if eta == 0:
            return np.zeros(nc, D)
        inv_eta = D(1) / eta
        s = D(0)
        for i in range(k, nr):
            A[i, k] = A[i, k] * inv_eta
            s = s + A[i, k] * A[i, k]
        sigma = np.sqrt(s)
        if A[k, k] < 0:
            sigma = -sigma
        A[k, k] = A[k, k] + sigma
        A1[k] = sigma * A[k, k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            sm = D(0)
            for i in range(k, nr):
                sm = sm + A[i, k] * A[i, j]
            tau = sm / A1[k]
            for i in range(k, nr):
                A[i, j] = A[i, j] - tau * A[i, k]
    for j in range(nc):
        tau = D(0)
        for i in range(j, nr):
            tau = tau + A[i, j] * b[i]
        tau = tau / A1[j]
        for i in range(j, nr):
            b[i] = b[i] - tau * A[i, j]
    X = np.zeros(nc, D)
    X[nc - 1] = b[nc - 1] / A2[nc - 1]
    for i in range(nc - 2, -1, -1):
        s = D(0)
        for j in range(i + 1, nc):
            s = s + A[i, j] * X[j]
        X[i] = (b[i] - s) / A2[i]
    return X


def jacobi_svd3(g):
    """cvSVD of the general 3x3 ABt as F13 fixes it: (U, V)"""
    G = np.array(g, D)
    V = np.eye(3, dtype=D)
    for _ in range(SWEEPS):
        rotated = False
        for p in range(2):
            for q in range(p + 1, 3):
                gp, gq = G[:, p].copy(), G[:, q].copy()
                alpha = (gp[0] * gp[0] + gp[1] * gp[1]) + gp[2] * gp[2]
                beta = (gq[0] * gq[0] + gq[1] * gq[1]) + gq[2] * gq[2]
                gamma = (gp[0] * gq[0] + gp[1] * gq[1]) + gp[2] * gq[2]
                if gamma * gamma > SVD_EPS * (alpha * beta):
                    rotated = True
                    zeta = (beta - alpha) / (D(2) * gamma)
                    den = np.abs(zeta) + np.sqrt(zeta * zeta + D(1))
                    t = (D(-1) if zeta < 0.0 else D(1)) / den
                    c = D(1) / np.sqrt(t * t + D(1))
                    s = t * c
                    G[:, p] = c * gp - s * gq
                    G[:, q] = s * gp + c * gq
                    vp, vq = V[:, p].copy(), V[:, q].copy()
                    V[:, p] = c * vp - s * vq
                    V[:, q] = s * vp + c * vq
        if not rotated:
            break
    sv = np.array([np.sqrt((G[0, j] * G[0, j] + G[1, j] * G[1, j]) + G[2, j] * G[2, j]) for j in range(3)], D)
    for i in range(2):
        m = i
        for j in range(i + 1, 3):
            if sv[j] > sv[m]:
                m = j
        if m != i:
            sv[[i, m]] = sv[[m, i]]
            G[:, [i, m]] = G[:, [m, i]]
            V[:, [i, m]] = V[:, [m, i]]
    G[:, 0] = G[:, 0] / sv[0]
    G[:, 1] = G[:, 1] / sv[1]
    if sv[2] <= RANK_EPS * sv[0]:
        def cross(a, b):
            return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], D)
        G[:, 2] = cross(G[:, 0], G[:, 1])
        V[:, 2] = cross(V[:, 0], V[:, 1])
    else:
        G[:, 2] = G[:, 2] / sv[2]
    return G, V


class Own:
    """the library's primitives"""
    name = "own"
    eig = staticmethod(jacobi_eig)
    inv3 = staticmethod(adjugate_inverse)
    lstsq = staticmethod(qr_solve)
    svd3 = staticmethod(jacobi_svd3)


class Lapack:
    """the LAPACK variant: numpy.linalg for the OpenCV-owned primitives.  Where LAPACK gives up (a singular or non-finite
    matrix) the result is NaN, which the rest of the source carries to an empty mask."""
    name = "lapack"

    @staticmethod
    def _nan(call, arg, *shapes):
        try:
            if np.isfinite(arg).all():
                return call()
        except np.linalg.LinAlgError:
            pass
        out = [np.full(s, np.nan, D) for s in shapes]
        return out[0] if len(out) == 1 else tuple(out)

    @staticmethod
    def eig(a):
        a = np.array(a, D)
        d = a.shape[0]

        def call():
            w, V = np.linalg.eigh(a)
            return w[::-1].copy(), V[:, ::-1].copy()
        return Lapack._nan(call, a, d, (d, d))

    @staticmethod
    def inv3(c):
        return Lapack._nan(lambda: np.linalg.inv(np.array(c, D)), np.array(c, D), (3, 3))

    @staticmethod
    def lstsq(A, b):
        A = np.array(A, D)
        return Lapack._nan(lambda: np.linalg.lstsq(A, np.array(b, D), rcond=None)[0], np.append(A.reshape(-1), b), A.shape[1])

    @staticmethod
    def svd3(g):
        def call():
            U, _, Vt = np.linalg.svd(np.array(g, D))
            return U, Vt.T.copy()
        return Lapack._nan(call, np.array(g, D), (3, 3), (3, 3))


# ------------------------------------------------------------------------------------------------ EPnP
class Epnp:
    """compute_pose for the correspondences pws [n, 3], us [n, 2] (floats widened, as add_correspondence does)"""

    def __init__(self, pws, us, camera, prim=Own):
        self.pws = np.array(pws, D).reshape(-1, 3)
        self.us = np.array(us, D).reshape(-1, 2)
        self.n = len(self.pws)
        self.fu, self.fv, self.uc, self.vc = (D(c) for c in camera)
        self.prim = prim

    def choose_control_points(self):
        n = self.n
        c0 = np.zeros(3, D)
        for i in range(n):
            c0 = c0 + self.pws[i]
        c0 = c0 / D(n)
        a = np.zeros((3, 3), D)
        for i in range(n):                       # cvMulTransposed(PW0, ., 1): rows in ascending order
            d = self.pws[i] - c0
            a = a + np.outer(d, d)
        dc, V = self.prim.eig(a)
        self.cws = np.zeros((4, 3), D)
        self.cws[0] = c0
        for i in range(1, 4):
            k = np.sqrt(dc[i - 1] / D(n))
            self.cws[i] = c0 + k * V[:, i - 1]

    def compute_barycentric_coordinates(self):
        cc = np.zeros((3, 3), D)
        for i in range(3):
            for j in range(1, 4):
                cc[i, j - 1] = self.cws[j, i] - self.cws[0, i]
        ci = self.prim.inv3(cc)
        self.alphas = np.zeros((self.n, 4), D)
        for i in range(self.n):
            d = self.pws[i] - self.cws[0]
            for j in range(3):
                self.alphas[i, 1 + j] = (ci[j, 0] * d[0] + ci[j, 1] * d[1]) + ci[j, 2] * d[2]
            self.alphas[i, 0] = ((D(1) - self.alphas[i, 1]) - self.alphas[i, 2]) - self.alphas[i, 3]

    def fill_M(self, i):
        """the two rows of M of correspondence i"""
        a = self.alphas[i]
        m1 = np.zeros(12, D)
        m2 = np.zeros(12, D)
        m1[0::3] = a * self.fu
        m1[2::3] = a * (self.uc - self.us[i, 0])
        m2[1::3] = a * self.fv
        m2[2::3] = a * (self.vc - self.us[i, 1])
        return m1, m2

    def mtm(self):
        a = np.zeros((12, 12), D)
        for i in range(self.n):                  # cvMulTransposed(M, MtM, 1): rows in ascending order
            for m in self.fill_M(i):
                a = a + np.outer(m, m)
        return a

    def compute_L_6x10(self):
        v = [self.V[:, 11 - i] for i in range(4)]
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        L = np.zeros((6, 10), D)

        def dot(x, y):
            return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]
        for j, (a, b) in enumerate(pairs):
            dv = [v[i][3 * a:3 * a + 3] - v[i][3 * b:3 * b + 3] for i in range(4)]
            L[j] = [dot(dv[0], dv[0]), D(2) * dot(dv[0], dv[1]), dot(dv[1], dv[1]), D(2) * dot(dv[0], dv[2]),
                    D(2) * dot(dv[1], dv[2]), dot(dv[2], dv[2]), D(2) * dot(dv[0], dv[3]), D(2) * dot(dv[1], dv[3]),
                    D(2) * dot(dv[2], dv[3]), dot(dv[3], dv[3])]
        self.L = L

    def compute_rho(self):
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        rho = np.zeros(6, D)
        for j, (a, b) in enumerate(pairs):
            e = self.cws[a] - self.cws[b]
            rho[j] = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        self.rho = rho

    def find_betas_approx_1(self):
        x = self.prim.lstsq(self.L[:, [0, 1, 3, 6]], self.rho)
        if x[0] < 0:
            b0 = np.sqrt(-x[0])
            return np.array([b0, -x[1] / b0, -x[2] / b0, -x[3] / b0], D)
        b0 = np.sqrt(x[0])
        return np.array([b0, x[1] / b0, x[2] / b0, x[3] / b0], D)

    def _betas_23(self, x):
        if x[0] < 0:
            b0 = np.sqrt(-x[0])
            b1 = np.sqrt(-x[2]) if x[2] < 0 else D(0)
        else:
            b0 = np.sqrt(x[0])
            b1 = np.sqrt(x[2]) if x[2] > 0 else D(0)
        if x[1] < 0:
            b0 = -b0
        return b0, b1

    def find_betas_approx_2(self):
        x = self.prim.lstsq(self.L[:, [0, 1, 2]], self.rho)
        b0, b1 = self._betas_23(x)
        return np.array([b0, b1, 0, 0], D)

    def find_betas_approx_3(self):
        x = self.prim.lstsq(self.L[:, [0, 1, 2, 3, 4]], self.rho)
        b0, b1 = self._betas_23(x)
        return np.array([b0, b1, x[3] / b0, 0], D)

    def compute_A_and_b_gauss_newton(self, betas):
        b0, b1, b2, b3 = betas
        A = np.zeros((6, 4), D)
        b = np.zeros(6, D)
        for i in range(6):
            l0, l1, l2, l3, l4, l5, l6, l7, l8, l9 = self.L[i]
            A[i, 0] = (((D(2) * l0) * b0 + l1 * b1) + l3 * b2) + l6 * b3
            A[i, 1] = ((l1 * b0 + (D(2) * l2) * b1) + l4 * b2) + l7 * b3
            A[i, 2] = ((l3 * b0 + l4 * b1) + (D(2) * l5) * b2) + l8 * b3
            A[i, 3] = ((l6 * b0 + l7 * b1) + l8 * b2) + (D(2) * l9) * b3
            b[i] = self.rho[i] - ((((((((((l0 * b0) * b0 + (l1 * b0) * b1) + (l2 * b1) * b1) + (l3 * b0) * b2) + (l4 * b1) * b2) +
                                      (l5 * b2) * b2) + (l6 * b0) * b3) + (l7 * b1) * b3) + (l8 * b2) * b3) + (l9 * b3) * b3)
        return A, b

    def gauss_newton(self, betas):
        betas = np.array(betas, D)
        for _ in range(5):
            A, b = self.compute_A_and_b_gauss_newton(betas)
            betas = betas + qr_solve(A, b)           # the source's own routine in both modes
        return betas

    def compute_ccs(self, betas):
        ccs = np.zeros(12, D)
        for i in range(4):
            ccs = ccs + betas[i] * self.V[:, 11 - i]
        return ccs.reshape(4, 3)

    def compute_pcs(self, ccs):
        a = self.alphas
        return np.array([((a[i, 0] * ccs[0] + a[i, 1] * ccs[1]) + a[i, 2] * ccs[2]) + a[i, 3] * ccs[3] for i in range(self.n)], D)

    @staticmethod
    def solve_for_sign(ccs, pcs):
        if pcs[0, 2] < 0.0:
            return -ccs, -pcs
        return ccs, pcs

    def estimate_R_and_t(self, pcs):
        n = self.n
        pc0 = np.zeros(3, D)
        pw0 = np.zeros(3, D)
        for i in range(n):
            pc0 = pc0 + pcs[i]
            pw0 = pw0 + self.pws[i]
        pc0 = pc0 / D(n)
        pw0 = pw0 / D(n)
        abt = np.zeros((3, 3), D)
        for i in range(n):
            abt = abt + np.outer(pcs[i] - pc0, self.pws[i] - pw0)
        U, V = self.prim.svd3(abt)
        R = np.zeros((3, 3), D)
        for i in range(3):
            for j in range(3):
                R[i, j] = (U[i, 0] * V[j, 0] + U[i, 1] * V[j, 1]) + U[i, 2] * V[j, 2]
        det = (((((R[0, 0] * R[1, 1]) * R[2, 2] + (R[0, 1] * R[1, 2]) * R[2, 0]) + (R[0, 2] * R[1, 0]) * R[2, 1]) -
                (R[0, 2] * R[1, 1]) * R[2, 0]) - (R[0, 1] * R[1, 0]) * R[2, 2]) - (R[0, 0] * R[1, 2]) * R[2, 1]
        if det < 0:
            R[2] = -R[2]
        t = np.array([pc0[i] - ((R[i, 0] * pw0[0] + R[i, 1] * pw0[1]) + R[i, 2] * pw0[2]) for i in range(3)], D)
        return R, t

    def reprojection_error(self, R, t):
        s = D(0)
        for i in range(self.n):
            x, y, z = self.pws[i]
            Xc = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0]
            Yc = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1]
            inv_Zc = D(1) / (((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2])
            ue = self.uc + (self.fu * Xc) * inv_Zc
            ve = self.vc + (self.fv * Yc) * inv_Zc
            du, dv = self.us[i, 0] - ue, self.us[i, 1] - ve
            s = s + np.sqrt(du * du + dv * dv)
        return s / D(self.n)

    def compute_R_and_t(self, betas):
        ccs = self.compute_ccs(betas)
        pcs = self.compute_pcs(ccs)
        ccs, pcs = self.solve_for_sign(ccs, pcs)
        R, t = self.estimate_R_and_t(pcs)
        return R, t, self.reprojection_error(R, t)

    def compute_pose(self):
        """-> (R, t, N)"""
        with np.errstate(all="ignore"):
            self.choose_control_points()
            self.compute_barycentric_coordinates()
            _, self.V = self.prim.eig(self.mtm())
            self.compute_L_6x10()
            self.compute_rho()
            res = {}
            for N, approx in ((1, self.find_betas_approx_1), (2, self.find_betas_approx_2), (3, self.find_betas_approx_3)):
                res[N] = self.compute_R_and_t(self.gauss_newton(approx()))
            N = 1
            if res[2][2] < res[1][2]:
                N = 2
            if res[3][2] < res[N][2]:
                N = 3
            return res[N][0], res[N][1], N


def canon(x):
    """a stored NaN is the canonical quiet NaN"""
    x = np.array(x)
    x[np.isnan(x)] = np.nan
    return x


def to_Tcw(R, t):
    """what iterate() / Refine() make of mRi, mti: eye(4) with the float conversions"""
    with np.errstate(all="ignore"):
        T = np.eye(4, dtype=F)
        T[:3, :3] = canon(R).astype(F)
        T[:3, 3] = canon(t).astype(F)
    return canon(T)


def check_inliers(R, t, camera, p3dw, p2d, max_err):
    """(:444-481) with the source's mixed widths -> bool mask"""
    fu, fv, uc, vc = (D(c) for c in camera)
    p3 = np.asarray(p3dw, F).reshape(-1, 3)
    p2 = np.asarray(p2d, F).reshape(-1, 2)
    with np.errstate(all="ignore"):
        x, y, z = (p3[:, c].astype(D) for c in range(3))
        Xc = (((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0]).astype(F)
        Yc = (((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1]).astype(F)
        invZc = (D(1) / (((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2])).astype(F)
        ue = uc + (fu * Xc.astype(D)) * invZc.astype(D)
        ve = vc + (fv * Yc.astype(D)) * invZc.astype(D)
        dx = (p2[:, 0].astype(D) - ue).astype(F)
        dy = (p2[:, 1].astype(D) - ve).astype(F)
        e2 = dx * dx + dy * dy
        return e2 < np.asarray(max_err, F)


class Hyp:
    """one evaluated iteration (or Refine): the double R, t, the float Tcw, the chosen N, the mask and its count"""

    def __init__(self, problem, idx, prim=Own):
        p3 = np.asarray(problem["p3dw"], F).reshape(-1, 3)
        p2 = np.asarray(problem["p2d"], F).reshape(-1, 2)
        R, t, N = Epnp(p3[idx], p2[idx], problem["camera"], prim).compute_pose()
        self.R, self.t, self.N = canon(R), canon(t), N
        self.Tcw = to_Tcw(R, t)
        self.mask = check_inliers(self.R, self.t, problem["camera"], p3, p2, problem["max_err"])
        self.count = int(self.mask.sum())


class Solver:
    """PnPsolver after SetRansacParameters: iterate() (:258-383) and Refine() (:386-438) over draws handed in as sets"""

    def __init__(self, problem, prim=Own, cache=None):
        self.p = problem
        self.prim = prim
        self.cache = cache if cache is not None else {}      # index tuple -> Hyp, shared between solvers on the same points
        self.n = len(np.asarray(problem["p3dw"]).reshape(-1, 3))
        self.min_inliers = int(problem["min_inliers"])
        self.max_its = int(problem["iterations"])
        self.sets = [tuple(int(v) for v in s) for s in np.asarray(problem["sets"], np.int32).reshape(-1, 4)] \
            if problem.get("sets") is not None else []
        self.hyps = {}
        self.done = 0
        self.best_inliers = 0
        self.best = None
        self.refined = {}

    def append(self, sets):
        self.sets += [tuple(int(v) for v in s) for s in np.asarray(sets, np.int32).reshape(-1, 4)]

    def _eval(self, idx):
        key = tuple(int(i) for i in idx)
        if key not in self.cache:
            self.cache[key] = Hyp(self.p, list(key), self.prim)
        return self.cache[key]

    def hyp(self, i):
        return self._eval(self.sets[i])

    def refine(self):
        return self._eval(np.flatnonzero(self.best.mask))

    def iterate(self, n_iterations):
        """-> (Tcw or None, no_more, inliers, ninliers), or None with the state unchanged when the call needs more sets than
        the solver has (the library's -2)"""
        state = (self.done, self.best_inliers, self.best, getattr(self, "best_it", -1))
        try:
            return self._iterate(n_iterations)
        except IndexError:
            self.done, self.best_inliers, self.best, self.best_it = state
            return None

    def _iterate(self, n_iterations):
        none = np.zeros(self.n, bool)
        if self.n < self.min_inliers:
            return None, True, none, 0
        cur = 0
        while self.done < self.max_its or cur < n_iterations:
            cur += 1
            i = self.done
            if i >= len(self.sets):
                raise IndexError
            self.done += 1
            h = self.hyp(i)
            if h.count >= self.min_inliers:
                if h.count > self.best_inliers:
                    self.best_inliers, self.best, self.best_it = h.count, h, i
                r = self.refine()
                if r.count > self.min_inliers:
                    return r.Tcw, False, r.mask, r.count
        if self.done >= self.max_its:
            if self.best_inliers >= self.min_inliers:
                return self.best.Tcw, True, self.best.mask, self.best_inliers
            return None, True, none, 0
        return None, False, none, 0
