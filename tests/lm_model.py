"""What g2o executes around one free vertex with a dense N x N system, restated in numpy float64 independent of csrc/orbx_lm.h:
the unpivoted L D L^T solve and OptimizationAlgorithmLevenberg::solve inside SparseOptimizer::optimize.  pose_model.py (N = 6)
and sim3opt_model.py (N = 7) supply the edges and the vertex.  Every operation is an IEEE double operation in the written
order."""
import numpy as np

F64 = np.float64
DBL_MAX = F64(np.finfo(np.float64).max)


def solve(N, H, lam, b):
    """(H + lam I) x = b, H[(j, k)] for j <= k, unpivoted L D L^T; solved when every pivot is > 0 and finite, otherwise (False, 0)"""
    A = [[(H[(min(i, j), max(i, j))] + lam) if i == j else H[(min(i, j), max(i, j))] for j in range(N)] for i in range(N)]
    L = [[F64(0)] * N for _ in range(N)]
    d = [F64(0)] * N
    ok = True
    for j in range(N):
        w = [L[j][k] * d[k] for k in range(j)]
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * w[k]
        d[j] = s
        if not (s > 0 and s <= DBL_MAX):
            ok = False
        for i in range(j + 1, N):
            t = A[i][j]
            for k in range(j):
                t = t - L[i][k] * w[k]
            L[i][j] = t / s
    if not ok:
        return False, [F64(0)] * N
    y = [F64(0)] * N
    for i in range(N):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    x = [F64(0)] * N
    for i in range(N - 1, -1, -1):
        s = y[i] / d[i]
        for k in range(i + 1, N):
            s = s - L[k][i] * x[k]
        x[i] = s
    return True, x


def levenberg(N, iters, est, system, chi, oplus, on_iter=None):
    """SparseOptimizer::optimize(iters) -> (est, last); last = where computeActiveErrors ran last (a rejected last trial included).
    system(est) -> (H, b, chi, extra); chi(est) -> chi; oplus(est, x) -> est (may write x: computeScale reads it afterwards).
    on_iter(it, record, est, extra) is called once per iteration after system() with that iteration's trace record
    {"trials": [{"ok", "rho", "accepted", "nu", "chi"}, ...], "end": "ok" | "trials" | "rho0" | "stall"}, filled in as it runs."""
    last = est
    third, two_thirds = F64(1) / F64(3), F64(2) / F64(3)
    lam, nu, stall = F64(0), F64(2), 0
    for it in range(iters):
        H, b, cur, extra = system(est)
        last = est
        ini = cur
        itr = {"trials": [], "end": "ok"}
        if on_iter is not None:
            on_iter(it, itr, est, extra)
        if it == 0:                                  # computeLambdaInit
            m = F64(0)
            for j in range(N):
                a = np.abs(H[(j, j)])
                m = m if a < m else a
            lam, nu, stall = F64(1e-5) * m, F64(2), 0
        rho = F64(0)
        q = 0
        while True:
            backup = est
            ok, x = solve(N, H, lam, b)
            est = oplus(est, x)
            tmp = chi(est)
            last = est
            if not ok:
                tmp = DBL_MAX
            rho = cur - tmp
            scale = F64(0)
            for j in range(N):
                scale = scale + x[j] * (lam * x[j] + b[j])
            scale = scale + F64(1e-3)
            rho = rho / scale
            accepted = bool(rho > 0 and np.isfinite(tmp))
            itr["trials"].append({"ok": ok, "rho": float(rho), "accepted": accepted, "nu": float(nu), "chi": float(tmp)})
            if accepted:
                r2 = F64(2) * rho - F64(1)
                alpha = F64(1) - (r2 * r2) * r2
                alpha = two_thirds if two_thirds < alpha else alpha
                sf = alpha if third < alpha else third
                lam = lam * sf
                nu = F64(2)
                cur = tmp
            else:
                lam = lam * nu
                nu = nu * F64(2)
                est = backup
            q += 1
            if not (rho < 0 and q < 10):
                break
        if q == 10 or rho == 0:                      # Terminate
            itr["end"] = "trials" if q == 10 else "rho0"
            break
        if (ini - cur) * F64(1e3) < ini:
            stall += 1
        else:
            stall = 0
        if stall >= 3:                               # Stop criterium (Raul)
            itr["end"] = "stall"
            break
    return est, last
