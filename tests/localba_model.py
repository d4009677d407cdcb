"""Optimizer::LocalBundleAdjustment (src/Optimizer.cc:710-991) restated in numpy float64 from the reference, the g2o sources
(types_six_dof_expmap.cpp:103-234, base_binary_edge.hpp constructQuadraticForm, block_solver.hpp:354-486,
optimization_algorithm_levenberg.cpp) and DESIGN.md section 2 (F19), independently of csrc/orbx_localba.h: arrays over all edges
and all points, sums written as the orders F19 states.  The SE3 pieces come from tests/pose_model.py (F11), sin and cos from
the library (orbx_pose_sin_cos), as pose_model takes them.  Every elementwise numpy operation is one IEEE double operation, so
the results compare bit for bit with the library's host path and the device."""
import numpy as np

import pose_model as pm
from pose_model import F32, F64

CHI2_MONO, CHI2_STEREO = F64(5.991), F64(7.815)
CHAINS = 64
DBL_MAX = np.finfo(np.float64).max
# (j, k), j <= k, of a 6 x 6 upper triangle stored row by row
TRI6 = [(j, k) for j in range(6) for k in range(j, 6)]
TRI3 = [(a, b) for a in range(3) for b in range(a, 3)]


class State:
    def __init__(self, p, est=None):
        self.nlocal = int(p["nlocal"])
        T = np.asarray(p["Tcw"], np.float32).reshape(-1, 16)
        self.nkf = len(T)
        lf = np.asarray(p.get("local_fixed", np.zeros(self.nlocal)), bool)
        self.K = tuple(F64(v) for v in np.asarray(p["camera"], np.float32)) + (F64(F32(p["bf"])),)
        world = np.asarray(p["world"], np.float32).reshape(-1, 3)
        self.npts = len(world)
        self.begin = np.asarray(p["obs_begin"], np.int64)
        self.deg = np.diff(self.begin)
        self.nobs = int(self.begin[-1])
        self.kf = np.asarray(p["obs_kf"], np.int64).reshape(-1)
        obs = np.asarray(p["obs"], np.float32).reshape(-1, 3)
        self.ox, self.oy, self.our = (obs[:, i].astype(F64) for i in range(3))
        self.stereo = ~(obs[:, 2] < 0)
        self.w = np.asarray(p["inv_sigma2"], np.float32).astype(F64).reshape(-1)
        self.ept = np.repeat(np.arange(self.npts), self.deg)
        self.fcol = np.full(self.nkf, -1, np.int64)
        free = [i for i in range(self.nlocal) if not lf[i]]
        self.free = np.array(free, np.int64)
        self.fcol[self.free] = np.arange(len(free))
        self.nfree = len(free)
        self.efree = self.fcol[self.kf] >= 0 if self.nobs else np.zeros(0, bool)
        self.kf_list = [np.nonzero(self.fcol[self.kf] == f)[0] for f in range(self.nfree)]
        self.second_round = bool(p.get("second_round", True))
        Tsrc = T if est is None else np.asarray(est[0], np.float32).reshape(-1, 16)
        wsrc = world if est is None else np.asarray(est[1], np.float32).reshape(-1, 3)
        self.q = np.zeros((self.nkf, 4)); self.t = np.zeros((self.nkf, 3))
        for i in range(self.nkf):
            q, t = pm.to_se3quat(Tsrc[i])
            self.q[i], self.t[i] = q, t
        self.pt = wsrc.astype(F64)
        self.flag = np.zeros(self.nobs, bool)
        self.echi = np.zeros(self.nobs)
        self.th = np.where(obs[:, 2] < 0, CHI2_MONO, CHI2_STEREO)

    # ------------------------------------------------------------------------------------------- edges
    def errors(self):
        """computeError + chi2 of every edge at the current estimates: (pc, err, chi2)"""
        q = tuple(self.q[self.kf, i] for i in range(4))
        t = tuple(self.t[self.kf, i] for i in range(3))
        X = self.pt[self.ept]
        e = pm.Edges(np.arange(self.nobs), self.ox, self.oy, self.our, self.w, X[:, 0], X[:, 1], X[:, 2], self.stereo)
        return pm._error((q, t), self.K, e)

    def depth_positive(self):
        q = tuple(self.q[self.kf, i] for i in range(4))
        X = self.pt[self.ept]
        return pm._rotate(q, X[:, 0], X[:, 1], X[:, 2])[2] + self.t[self.kf, 2] > 0

    def jacobians(self, pc):
        """linearizeOplus: Ji [3][3] by the point, Jx [3][6] by the pose, lists of arrays over the edges"""
        fx, fy, cx, cy, bf = self.K
        q = tuple(self.q[self.kf, i] for i in range(4))
        R = pm._R_from_quat(q)
        x, y, z = pc
        z_2 = z * z
        st = self.stereo
        one = F64(1)
        m = -one / z
        a00, a02, a11, a12 = m * fx, m * ((-x / z) * fx), m * fy, m * ((-y / z) * fy)
        Ji = [[None] * 3 for _ in range(3)]
        for a in range(3):
            s0 = (-fx * R[0][a]) / z + ((fx * x) * R[2][a]) / z_2
            s1 = (-fy * R[1][a]) / z + ((fy * y) * R[2][a]) / z_2
            Ji[0][a] = np.where(st, s0, a00 * R[0][a] + a02 * R[2][a])
            Ji[1][a] = np.where(st, s1, a11 * R[1][a] + a12 * R[2][a])
            Ji[2][a] = np.where(st, s0 - (bf * R[2][a]) / z_2, F64(0))
        zero = np.zeros_like(z)
        Jx = [[((x * y) / z_2) * fx, -(one + ((x * x) / z_2)) * fx, (y / z) * fx, (-one / z) * fx, zero, (x / z_2) * fx],
              [(one + (y * y) / z_2) * fy, ((-x * y) / z_2) * fy, (-x / z) * fy, zero, (-one / z) * fy, (y / z_2) * fy]]
        Jx.append([np.where(st, Jx[0][0] - (bf * y) / z_2, zero), np.where(st, Jx[0][1] + (bf * x) / z_2, zero),
                   np.where(st, Jx[0][2], zero), np.where(st, Jx[0][3], zero), zero, np.where(st, Jx[0][5] - bf / z_2, zero)])
        return Ji, Jx

    def rows(self, r0, r1, r2):
        s = r0 + r1
        return np.where(self.stereo, s + r2, s)

    # ------------------------------------------------------------------------------------------- ordered sums
    def by_point(self, terms, sign, init=None):
        """per point: acc = acc (+|-) term over the point's active edges in CSR order; terms [nobs, m]"""
        acc = np.zeros((self.npts, terms.shape[1])) if init is None else init.copy()
        for j in range(int(self.deg.max()) if self.npts else 0):
            valid = j < self.deg
            e = np.where(valid, self.begin[:-1] + j, 0)
            act = valid & ~self.flag[e] & self.emask[e]
            nxt = acc + terms[e] if sign > 0 else acc - terms[e]
            acc = np.where(act[:, None], nxt, acc)
        return acc

    def by_keyframe(self, terms, minus_from=None):
        """per free keyframe: 64 interleaved chains over its edge list (ascending edge index), the partials added in order of the
        chain.  Columns from minus_from on are subtracted inside a chain (b -= ...)."""
        m = terms.shape[1]
        out = np.zeros((self.nfree, m))
        for f, L in enumerate(self.kf_list):
            steps = -(-len(L) // CHAINS)
            pad = np.full(steps * CHAINS, -1, np.int64)
            pad[:len(L)] = L
            pad = pad.reshape(steps, CHAINS)
            a = np.zeros((CHAINS, m))
            for s in range(steps):
                e = pad[s]
                es = np.where(e >= 0, e, 0)
                act = (e >= 0) & ~self.flag[es]
                nxt = a + terms[es]
                if minus_from is not None:
                    nxt[:, minus_from:] = a[:, minus_from:] - terms[es][:, minus_from:]
                a = np.where(act[:, None], nxt, a)
            tot = np.zeros(m)
            for c in range(CHAINS):
                tot = tot + a[c]
            out[f] = tot
        return out

    def chain_reduce(self, n, step):
        """64 chains over items 0..n-1 (chain c takes c, c + 64, ...): acc = step(acc, items, valid) per stride, then the partials
        go through the caller's combine"""
        acc = np.zeros(CHAINS)
        for s in range(-(-n // CHAINS)):
            items = s * CHAINS + np.arange(CHAINS)
            valid = items < n
            acc = step(acc, np.where(valid, items, 0), valid)
        return acc

    def chi_total(self, cp):
        def step(acc, p, valid):
            return np.where(valid, acc + cp[p], acc)
        red = self.chain_reduce(self.npts, step) if self.npts else np.zeros(CHAINS)
        s = F64(0)
        for c in range(CHAINS):
            s = s + red[c]
        return s

    # ------------------------------------------------------------------------------------------- one linearisation
    def activity(self):
        self.emask = np.ones(self.nobs, bool)
        act = ~self.flag
        self.pact = np.array([act[self.begin[p]:self.begin[p + 1]].any() for p in range(self.npts)], bool)
        kact = np.array([act[L].any() for L in self.kf_list], bool)
        self.ccol = np.where(kact, np.cumsum(kact) - 1, -1)
        self.nact = int(kact.sum())
        return bool(self.pact.any())

    def active_chi(self, robust, system=False):
        """computeActiveErrors + activeRobustChi2 [+ buildSystem]"""
        pc, err, chi2 = self.errors()
        act = ~self.flag
        self.echi = np.where(act, chi2, self.echi)
        rho0, rho1 = pm._huber(chi2, self.stereo, robust)
        cp = self.by_point(rho0[:, None], +1)[:, 0]
        total = self.chi_total(cp)
        if not system:
            return total
        Ji, Jx = self.jacobians(pc)
        W = rho1 * self.w
        we = [self.w * err[r] for r in range(3)]
        tH = np.stack([self.rows(*[(Ji[r][a] * W) * Ji[r][b] for r in range(3)]) for a, b in TRI3], 1)
        tb = np.stack([rho1 * self.rows(*[Ji[r][a] * we[r] for r in range(3)]) for a in range(3)], 1)
        self.Hll = self.by_point(tH, +1)
        self.bl = self.by_point(tb, -1)
        kH = [self.rows(*[(Jx[r][j] * W) * Jx[r][k] for r in range(3)]) for j, k in TRI6]
        kb = [rho1 * self.rows(*[Jx[r][j] * we[r] for r in range(3)]) for j in range(6)]
        self.Hpp = self.by_keyframe(np.stack(kH + kb, 1), minus_from=21) if self.nobs else np.zeros((self.nfree, 27))
        self.Hpl = np.stack([np.stack([self.rows(*[(Jx[r][j] * W) * Ji[r][a] for r in range(3)]) for a in range(3)], 1)
                             for j in range(6)], 1)                                   # [nobs, 6, 3]
        return total

    def max_diag(self):
        dk = [0, 6, 11, 15, 18, 20]
        m = np.zeros(CHAINS)

        def take(m, a, ok):
            return np.where(ok, np.where(a < m, m, a), m)
        for s in range(-(-self.nfree // CHAINS)):
            f = s * CHAINS + np.arange(CHAINS)
            ok = f < self.nfree
            fs = np.where(ok, f, 0)
            ok = ok & (self.ccol[fs] >= 0) if self.nfree else ok
            for d in dk:
                m = take(m, np.abs(self.Hpp[fs, d]) if self.nfree else m, ok)
        for s in range(-(-self.npts // CHAINS)):
            p = s * CHAINS + np.arange(CHAINS)
            ok = p < self.npts
            ps = np.where(ok, p, 0)
            ok = ok & self.pact[ps]
            for d in (0, 3, 5):
                m = take(m, np.abs(self.Hll[ps, d]), ok)
        r = F64(0)
        for c in range(CHAINS):
            r = m[c] if not (m[c] < r) else r
        return r

    def scale(self, lam):
        s = np.zeros(CHAINS)
        for st in range(-(-self.nfree // CHAINS)):
            f = st * CHAINS + np.arange(CHAINS)
            ok = f < self.nfree
            fs = np.where(ok, f, 0)
            cc = self.ccol[fs]
            ok = ok & (cc >= 0)
            cs = np.where(ok, cc, 0)
            for j in range(6):
                xv = self.x[6 * cs + j] if self.nact else np.zeros(CHAINS)
                s = np.where(ok, s + xv * (lam * xv + self.Hpp[fs, 21 + j]), s)
        for st in range(-(-self.npts // CHAINS)):
            p = st * CHAINS + np.arange(CHAINS)
            ok = p < self.npts
            ps = np.where(ok, p, 0)
            ok = ok & self.pact[ps]
            for j in range(3):
                xv = self.xl[ps, j]
                s = np.where(ok, s + xv * (lam * xv + self.bl[ps, j]), s)
        r = F64(0)
        for c in range(CHAINS):
            r = r + s[c]
        return r

    def reduced_system(self, lam):
        """Dinv, S (lower triangle filled) and b_s over the active free keyframes"""
        h = self.Hll
        a00, a01, a02, a11, a12, a22 = h[:, 0] + lam, h[:, 1], h[:, 2], h[:, 3] + lam, h[:, 4], h[:, 5] + lam
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        inv = F64(1) / det
        D = np.stack([np.stack([c00 * inv, c01 * inv, c02 * inv], 1), np.stack([c01 * inv, c11 * inv, c12 * inv], 1),
                      np.stack([c02 * inv, c12 * inv, c22 * inv], 1)], 1)             # [npts, 3, 3]
        b = self.bl
        self.Dinv = D
        self.Dbl = np.stack([(D[:, a, 0] * b[:, 0] + D[:, a, 1] * b[:, 1]) + D[:, a, 2] * b[:, 2] for a in range(3)], 1)
        H = self.Hpl
        De = D[self.ept]
        Y = np.stack([np.stack([(H[:, j, 0] * De[:, 0, a] + H[:, j, 1] * De[:, 1, a]) + H[:, j, 2] * De[:, 2, a] for a in range(3)], 1)
                      for j in range(6)], 1)
        nf = self.nfree
        S4 = np.zeros((nf, nf, 6, 6))
        for f in range(nf):
            for n, (j, k) in enumerate(TRI6):
                S4[f, f, j, k] = self.Hpp[f, n]
                S4[f, f, k, j] = self.Hpp[f, n]
            for j in range(6):
                S4[f, f, j, j] = S4[f, f, j, j] + lam
        live = ~self.flag & self.efree
        for p in range(self.npts):                             # ascending point order: every block gets its entries in order
            E = np.arange(self.begin[p], self.begin[p + 1])
            E = E[live[E]]
            if len(E) == 0:
                continue
            fa = self.fcol[self.kf[E]]
            Ya, Hb = Y[E][:, None, :, None, :], H[E][None, :, None, :, :]
            Wm = (Ya[..., 0] * Hb[..., 0] + Ya[..., 1] * Hb[..., 1]) + Ya[..., 2] * Hb[..., 2]      # [a, b, r, k]
            ia, ib = np.nonzero(fa[:, None] <= fa[None, :])
            S4[fa[ia], fa[ib]] = S4[fa[ia], fa[ib]] - Wm[ia, ib]
        n = 6 * self.nact
        A = np.zeros((n, n))
        actf = [f for f in range(nf) if self.ccol[f] >= 0]
        for i1 in actf:
            for i2 in actf:
                if i1 > i2:
                    continue
                c1, c2 = 6 * self.ccol[i1], 6 * self.ccol[i2]
                blk = S4[i1, i2].T
                A[c2:c2 + 6, c1:c1 + 6] = np.tril(blk) if i1 == i2 else blk
        t = np.stack([(H[:, r, 0] * self.Dbl[self.ept, 0] + H[:, r, 1] * self.Dbl[self.ept, 1]) + H[:, r, 2] * self.Dbl[self.ept, 2]
                      for r in range(6)], 1) if self.nobs else np.zeros((0, 6))
        sums = self.by_keyframe(t) if self.nobs else np.zeros((nf, 6))
        bs = np.zeros(n)
        for f in actf:
            bs[6 * self.ccol[f]:6 * self.ccol[f] + 6] = self.Hpp[f, 21:27] - sums[f]
        return A, bs

    def solve(self, lam):
        A, bs = self.reduced_system(lam)
        n = len(bs)
        L = np.tril(A, -1)
        d = np.zeros(n)
        for j in range(n):                                     # left-looking: rows i >= j, chains over k ascending
            col = A[j:, j].copy()
            for k in range(j):
                wv = L[j, k] * d[k]
                col = col - L[j:, k] * wv
            d[j] = col[0]
            L[j + 1:, j] = col[1:] / col[0]
        ok = bool(np.all((d > 0) & (d <= DBL_MAX)))
        x = np.zeros(n)
        if ok:
            y = bs.copy()
            for k in range(n - 1):
                y[k + 1:] = y[k + 1:] - L[k + 1:, k] * y[k]
            x = y / d
            for k in range(n - 1, 0, -1):
                x[:k] = x[:k] - L[k, :k] * x[k]
        self.x = x
        if not ok:
            self.xl = np.zeros((self.npts, 3))
            return False
        H = self.Hpl
        cc = np.where(self.efree, self.ccol[np.where(self.efree, self.fcol[self.kf], 0)], 0) if self.nobs and self.nfree else np.zeros(self.nobs, np.int64)
        s = np.zeros((self.nobs, 3))
        if n:
            xe = x[(6 * np.where(cc >= 0, cc, 0))[:, None] + np.arange(6)[None, :]]            # [nobs, 6]
            for a in range(3):
                sa = H[:, 0, a] * xe[:, 0]
                for j in range(1, 6):
                    sa = sa + H[:, j, a] * xe[:, j]
                s[:, a] = sa
        self.emask = self.efree
        v = self.by_point(s, -1, init=self.bl)
        self.emask = np.ones(self.nobs, bool)
        D = self.Dinv
        xl = np.stack([(D[:, a, 0] * v[:, 0] + D[:, a, 1] * v[:, 1]) + D[:, a, 2] * v[:, 2] for a in range(3)], 1)
        self.xl = np.where(self.pact[:, None], xl, 0.0)
        return True

    def update(self):
        self.backup = (self.q.copy(), self.t.copy(), self.pt.copy())
        for f in range(self.nfree):
            cc = self.ccol[f]
            if cc < 0:
                continue
            i = self.free[f]
            q, t = pm._mul(pm.se3_exp([F64(v) for v in self.x[6 * cc:6 * cc + 6]]), (tuple(self.q[i]), tuple(self.t[i])))
            self.q[i], self.t[i] = q, t
        self.pt = np.where(self.pact[:, None], self.pt + self.xl, self.pt)

    def restore(self):
        self.q, self.t, self.pt = self.backup

    def optimize(self, iters, robust, trace):
        """initializeOptimization(0) + optimize(iters) -> (iterations run, chi2 at the first linearisation, chi2 at the end)"""
        if not self.activity():
            return 0, F64(0), F64(0)
        lam, nu, stall, it = F64(0), F64(2), 0, 0
        first = cur = F64(0)
        while it < iters:
            cur = self.active_chi(robust, system=True)
            ini = cur
            if it == 0:
                first = cur
                lam = F64(1e-5) * self.max_diag()
                nu, stall = F64(2), 0
            it += 1
            q = 0
            while True:
                ok = self.solve(lam)
                self.update()
                tmp = self.active_chi(robust)
                if not ok:
                    tmp = F64(DBL_MAX)
                rho = cur - tmp
                rho = rho / (self.scale(lam) + F64(1e-3))
                accepted = bool(rho > 0 and np.isfinite(tmp))
                trace.append(("trial", robust, it, accepted, ok))
                if accepted:
                    r2 = F64(2) * rho - F64(1)
                    alpha = F64(1) - (r2 * r2) * r2
                    alpha = F64(2) / F64(3) if F64(2) / F64(3) < alpha else alpha
                    sf = alpha if F64(1) / F64(3) < alpha else F64(1) / F64(3)
                    lam, nu, cur = lam * sf, F64(2), tmp
                else:
                    lam, nu = lam * nu, nu * F64(2)
                    self.restore()
                q += 1
                if not (rho < 0 and q < 10):
                    break
            if q == 10 or rho == 0:
                break
            stall = stall + 1 if (ini - cur) * F64(1e3) < ini else 0
            if stall >= 3:
                break
        return it, first, cur

    def outliers(self, echi=None):
        echi = self.echi if echi is None else echi
        return (echi > self.th) | ~self.depth_positive()


def _canon(a):
    a = np.array(a)
    a[np.isnan(a)] = np.nan
    return a


def run(p, trace=None):
    """-> dict(Tcw [nlocal, 16] float32, world [npoints, 3] float32, erase uint8, iters, nflagged, nerase, chi2 [4])"""
    trace = [] if trace is None else trace
    with np.errstate(all="ignore"):
        s = State(p)
        iters, chi2 = [0, 0], [F64(0)] * 4
        iters[0], chi2[0], chi2[1] = s.optimize(5, True, trace)
        if s.second_round:
            fresh = s.errors()[2]
            s.flag = s.outliers()
            trace.append(("round1", int(np.sum(s.flag != ((fresh > s.th) | ~s.depth_positive()))),
                          int(np.sum(~(s.echi > s.th) & s.flag))))
            iters[1], chi2[2], chi2[3] = s.optimize(10, False, trace)
        erase = s.outliers()
        fresh = s.errors()[2]
        trace.append(("final", int(np.sum(s.flag & (erase != ((fresh > s.th) | ~s.depth_positive()))))))
        Tcw = np.stack([pm.to_cvmat((tuple(s.q[i]), tuple(s.t[i]))).reshape(16) for i in range(s.nlocal)]) if s.nlocal \
            else np.zeros((0, 16), np.float32)
        return dict(Tcw=_canon(Tcw.astype(np.float32)), world=_canon(s.pt.astype(np.float32)), erase=erase.astype(np.uint8),
                    iters=iters, nflagged=int(s.flag.sum()), nerase=int(erase.sum()), chi2=_canon(np.array(chi2, F64)))


def classify(p, Tcw_est, world_est, Tcw_last, world_last):
    """the classification alone: chi2 at the "last" estimates, isDepthPositive at the estimates"""
    with np.errstate(all="ignore"):
        last = State(p, (Tcw_last, world_last))
        chi2 = last.errors()[2]
        s = State(p, (Tcw_est, world_est))
        return s.outliers(chi2).astype(np.uint8)


def full_system(p, lam_scale=F64(1e-5)):
    """One linearisation at the start estimates for the sanity test of the Schur step: the full (6 nfree + 3 npoints) system
    (H + lambda I, b) as dense float64, and the model's Schur solution (x_p, x_l) of it."""
    with np.errstate(all="ignore"):
        s = State(p)
        s.activity()
        s.active_chi(True, system=True)
        lam = lam_scale * s.max_diag()
        assert s.solve(lam)
        n, m = 6 * s.nfree, 3 * s.npts
        Hf, bf = np.zeros((n + m, n + m)), np.zeros(n + m)
        for f in range(s.nfree):
            for k, (i, j) in enumerate(TRI6):
                Hf[6 * f + i, 6 * f + j] = Hf[6 * f + j, 6 * f + i] = s.Hpp[f, k]
            bf[6 * f:6 * f + 6] = s.Hpp[f, 21:27]
        for q in range(s.npts):
            for k, (i, j) in enumerate(TRI3):
                Hf[n + 3 * q + i, n + 3 * q + j] = Hf[n + 3 * q + j, n + 3 * q + i] = s.Hll[q, k]
            bf[n + 3 * q:n + 3 * q + 3] = s.bl[q]
        for e in np.nonzero(s.efree)[0]:
            f, q = s.fcol[s.kf[e]], s.ept[e]
            Hf[6 * f:6 * f + 6, n + 3 * q:n + 3 * q + 3] = s.Hpl[e]
            Hf[n + 3 * q:n + 3 * q + 3, 6 * f:6 * f + 6] = s.Hpl[e].T
        Hf = Hf + lam * np.eye(n + m)
        return Hf, bf, np.concatenate([s.x, s.xl.reshape(-1)])
