"""Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1050-1358) restated in numpy float64, independent of
csrc/orbx_essgraph.h: the measurements Sji = Sjw * Swi, EdgeSim3::computeError with g2o::Sim3::log, the numeric Jacobians of
BaseBinaryEdge::linearizeOplus (central differences, delta = 1e-9), the 7 x 7 block-sparse normal equations, the elimination
order in rounds of independent low-degree vertices, the block L D L^T held in Python dicts of 7 x 7 blocks,
OptimizationAlgorithmLevenberg::solve with setUserLambdaInit(1e-16), the recovery of Tiw and the correction of the points.
Every operation is an IEEE double operation in the written order (numpy elementwise arithmetic over the edges, the vertices
or the entries of a block is the same operation per element); every sum runs in the order DESIGN.md section 2 (F20) states.
The primitives taken from the library are exp (orbx_sim3opt_exp), sin / cos (orbx_pose_sin_cos) and atan2 (orbx_sim3_atan2),
as F11, F12 and F16 state; log is restated here.  `trace`, when given, receives what the tests assert branch coverage from."""
import ctypes as C

import numpy as np

F64 = np.float64
DELTA = F64(1e-9)
LAMBDA0 = F64(1e-16)
ITERS, TRIALS, CHAINS = 20, 10, 64
DBL_MAX = np.finfo(np.float64).max
CANON64 = np.uint64(0x7ff8000000000000)
CANON32 = np.uint32(0x7fc00000)
EPS = F64(0.00001)


def _lib():
    from orb_slam2_detailed_comments_amd import _capi
    return _capi.lib()


def _each(f, *arrs):
    a = [np.atleast_1d(np.asarray(v, F64)) for v in arrs]
    return [f(*(float(v[i]) for v in a)) for i in range(len(a[0]))]


def _sincos(theta):
    L = _lib()

    def f(t):
        s, c = C.c_double(), C.c_double()
        L.orbx_pose_sin_cos(t, C.byref(s), C.byref(c))
        return s.value, c.value
    r = np.array(_each(f, theta), F64).reshape(-1, 2)
    return r[:, 0], r[:, 1]


def _atan2(y, x):
    L = _lib()
    return np.array(_each(lambda a, b: L.orbx_sim3_atan2(a, b), y, x), F64)


def _exp(x):
    L = _lib()
    return np.array(_each(lambda a: L.orbx_sim3opt_exp(a), x), F64)


# ------------------------------------------------------------------------------------------------------------------- log
LN2_HI = F64(float.fromhex("0x1.62e42feep-1"))
LN2_LO = F64(float.fromhex("0x1.a39ef35793c76p-33"))
SQRT2 = F64(float.fromhex("0x1.6a09e667f3bcdp+0"))


def _log(x):
    """the library's log, elementwise: x = 2^k m, m in [sqrt(1/2), sqrt(2)], 2 atanh((m - 1) / (m + 1)) by its series; x < 0 and
    NaN give NaN, 0 gives -inf, +inf gives +inf"""
    x = np.atleast_1d(np.array(x, F64))
    with np.errstate(all="ignore"):
        tiny = x < F64(2.0) ** -1022
        xs = np.where(tiny, x * F64(2.0) ** 54, x)
        k = np.where(tiny, -54, 0).astype(np.int64)
        b = np.ascontiguousarray(xs).view(np.uint64)
        k = k + (b >> np.uint64(52)).astype(np.int64) - 1023
        m = ((b & np.uint64(0x000fffffffffffff)) | np.uint64(0x3ff0000000000000)).view(F64)
        big = m > SQRT2
        m = np.where(big, m * F64(0.5), m)
        k = np.where(big, k + 1, k)
        f = m - F64(1)
        s = f / (F64(2) + f)
        z = s * s
        p = np.full_like(z, F64(2) / F64(23))
        for n in (21, 19, 17, 15, 13, 11, 9, 7, 5, 3):
            p = p * z + F64(2) / F64(n)
        lm = F64(2) * s + (s * z) * p
        dk = k.astype(F64)
        r = dk * LN2_HI + (lm + dk * LN2_LO)
        r = np.where(x > 0, r, np.where(x == 0, F64(-np.inf), F64(np.nan)))
        return np.where(x <= DBL_MAX, r, np.where(x > 0, x, r))


def log1(x):
    return _log(x)[0]


# ------------------------------------------------------------------------------- g2o::Sim3 as [8, n]: q x y z w, t, s (arrays)
def _rotate(S, vx, vy, vz):
    qx, qy, qz, qw = S[0], S[1], S[2], S[3]
    ux, uy, uz = qy * vz - qz * vy, qz * vx - qx * vz, qx * vy - qy * vx
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return ((vx + qw * ux) + (qy * uz - qz * uy), (vy + qw * uy) + (qz * ux - qx * uz), (vz + qw * uz) + (qx * uy - qy * ux))


def _mul(A, B):
    v = _rotate(A, B[4], B[5], B[6])
    ax, ay, az, aw = A[0], A[1], A[2], A[3]
    bx, by, bz, bw = B[0], B[1], B[2], B[3]
    w = aw * bw - ax * bx - ay * by - az * bz
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by + ay * bw + az * bx - ax * bz
    z = aw * bz + az * bw + ax * by - ay * bx
    return np.stack([x, y, z, w, A[7] * v[0] + A[4], A[7] * v[1] + A[5], A[7] * v[2] + A[6], A[7] * B[7]])


def _inverse(A):
    qc = np.stack([-A[0], -A[1], -A[2], A[3]])
    m = F64(-1) / A[7]
    v = _rotate(qc, m * A[4], m * A[5], m * A[6])
    return np.stack([qc[0], qc[1], qc[2], qc[3], v[0], v[1], v[2], F64(1) / A[7]])


def _R_from_quat(S):
    """Quaterniond::toRotationMatrix: m[r][c] arrays"""
    qx, qy, qz, qw = S[0], S[1], S[2], S[3]
    tx, ty, tz = F64(2) * qx, F64(2) * qy, F64(2) * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    one = F64(1)
    return [[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]]


def _quat_from_R(m):
    """Eigen's Quaterniond(Matrix3d), all four branches computed and selected per element"""
    with np.errstate(all="ignore"):
        half, one = F64(0.5), F64(1)
        tr = m[0][0] + m[1][1] + m[2][2]
        t = np.sqrt(tr + one)
        w0 = half * t
        t = half / t
        q0 = ((m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t, w0)
        t = np.sqrt(m[0][0] - m[1][1] - m[2][2] + one)
        x1 = half * t
        t = half / t
        q1 = (x1, (m[1][0] + m[0][1]) * t, (m[2][0] + m[0][2]) * t, (m[2][1] - m[1][2]) * t)
        t = np.sqrt(m[1][1] - m[2][2] - m[0][0] + one)
        y2 = half * t
        t = half / t
        q2 = ((m[0][1] + m[1][0]) * t, y2, (m[2][1] + m[1][2]) * t, (m[0][2] - m[2][0]) * t)
        t = np.sqrt(m[2][2] - m[0][0] - m[1][1] + one)
        z3 = half * t
        t = half / t
        q3 = ((m[0][2] + m[2][0]) * t, (m[1][2] + m[2][1]) * t, z3, (m[1][0] - m[0][1]) * t)
    b0 = tr > 0
    b1 = ~b0 & (m[0][0] >= m[1][1]) & (m[0][0] >= m[2][2])
    b2 = ~b0 & ~b1 & (m[1][1] > m[0][0]) & (m[1][1] >= m[2][2])
    return [np.where(b0, q0[k], np.where(b1, q1[k], np.where(b2, q2[k], q3[k]))) for k in range(4)]


def sim3_exp(u):
    """Sim3(Vector7d), sim3.h:70-142; u [7, n]"""
    zero, one = np.zeros_like(u[0]), F64(1)
    o0, o1, o2, sigma = u[0], u[1], u[2], u[6]
    theta = np.sqrt(o0 * o0 + o1 * o1 + o2 * o2)
    Om = [[zero, -o2, o1], [o2, zero, -o0], [-o1, o0, zero]]
    s = _exp(sigma)
    Om2 = [[Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j] for j in range(3)] for i in range(3)]
    small = theta < EPS
    sn, cs = _sincos(theta)
    with np.errstate(all="ignore"):
        theta2 = theta * theta
        sigma2 = sigma * sigma
        A_st = (one - cs) / theta2
        B_st = (theta - sn) / (theta2 * theta)
        C_S = (s - one) / sigma
        A_Ss = ((sigma - one) * s + one) / sigma2
        B_Ss = ((F64(0.5) * sigma2 - sigma + one) * s) / (sigma2 * sigma)
        a, b = s * sn, s * cs
        c = theta2 + sigma2
        A_St = (a * sigma + (one - b) * theta) / (theta * c)
        B_St = ((C_S - ((b - one) * sigma + a * theta) / c) * one) / theta2
        ra, rb = sn / theta, (one - cs) / (theta * theta)
    ss = np.abs(sigma) < EPS
    A = np.where(ss, np.where(small, one / F64(2), A_st), np.where(small, A_Ss, A_St))
    B = np.where(ss, np.where(small, one / F64(6), B_st), np.where(small, B_Ss, B_St))
    Cc = np.where(ss, one, C_S)
    I = [[one if i == j else F64(0) for j in range(3)] for i in range(3)]
    with np.errstate(all="ignore"):
        R = [[np.where(small, (I[i][j] + Om[i][j]) + Om2[i][j], (I[i][j] + ra * Om[i][j]) + rb * Om2[i][j]) for j in range(3)] for i in range(3)]
        W = [[(A * Om[i][j] + B * Om2[i][j]) + Cc * I[i][j] for j in range(3)] for i in range(3)]
        t = [W[i][0] * u[3] + W[i][1] * u[4] + W[i][2] * u[5] for i in range(3)]
    q = _quat_from_R(R)
    return np.stack([q[0], q[1], q[2], q[3], t[0], t[1], t[2], s])


def _oplus(est, u, fix_scale):
    """VertexSim3Expmap::oplusImpl: zeroes update[6] in place under _fix_scale"""
    if fix_scale:
        u[6] = F64(0)
    return _mul(sim3_exp(u), est)


def _solve3(M):
    """W.lu().solve(t): [W | t] as 3 rows of 4 arrays; partial pivoting, the first row of largest |pivot|"""
    with np.errstate(all="ignore"):
        a0, a1, a2 = np.abs(M[0][0]), np.abs(M[1][0]), np.abs(M[2][0])
        p1 = a1 > a0
        best = np.where(p1, a1, a0)
        p2 = a2 > best
        p = np.where(p2, 2, np.where(p1, 1, 0))
        r0 = [np.where(p == 0, M[0][j], np.where(p == 1, M[1][j], M[2][j])) for j in range(4)]
        r1 = [np.where(p == 1, M[0][j], M[1][j]) for j in range(4)]
        r2 = [np.where(p == 2, M[0][j], M[2][j]) for j in range(4)]
        l1, l2 = r1[0] / r0[0], r2[0] / r0[0]
        r1 = [None] + [r1[j] - l1 * r0[j] for j in range(1, 4)]
        r2 = [None] + [r2[j] - l2 * r0[j] for j in range(1, 4)]
        sw = np.abs(r2[1]) > np.abs(r1[1])
        r1, r2 = [None] + [np.where(sw, r2[j], r1[j]) for j in range(1, 4)], [None] + [np.where(sw, r1[j], r2[j]) for j in range(1, 4)]
        l = r2[1] / r1[1]
        m22 = r2[2] - l * r1[2]
        m23 = r2[3] - l * r1[3]
        x2 = m23 / m22
        x1 = (r1[3] - r1[2] * x2) / r1[1]
        x0 = ((r0[3] - r0[1] * x1) - r0[2] * x2) / r0[0]
    return x0, x1, x2


def sim3_log(S, trace=None):
    """Sim3::log, sim3.h:148-230; S [8, n] -> [7, n]"""
    one = F64(1)
    sigma = _log(S[7])
    R = _R_from_quat(S)
    d = F64(0.5) * (((R[0][0] + R[1][1]) + R[2][2]) - one)
    dr = (R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1])
    near = d > one - EPS
    with np.errstate(all="ignore"):
        sq = np.sqrt(one - d * d)
        theta = np.where(near, F64(0), _atan2(sq, d))
        f = np.where(near, F64(0.5), theta / (F64(2) * sq))
        o = [f * dr[k] for k in range(3)]
        sn, cs = _sincos(np.where(near, F64(0), theta))
        s = S[7]
        theta2 = theta * theta
        sigma2 = sigma * sigma
        A_st = (one - cs) / theta2
        B_st = (theta - sn) / (theta2 * theta)
        C_S = (s - one) / sigma
        A_Ss = ((sigma - one) * s + one) / sigma2
        B_Ss = ((F64(0.5) * sigma2 - sigma + one) * s) / (sigma2 * sigma)
        a, b = s * sn, s * cs
        c = theta2 + sigma * sigma
        A_St = (a * sigma + (one - b) * theta) / (theta * c)
        B_St = ((C_S - ((b - one) * sigma + a * theta) / c) * one) / theta2
    ss = np.abs(sigma) < EPS
    if trace is not None:
        for a_, b_ in zip(np.atleast_1d(ss), np.atleast_1d(near)):
            trace.setdefault("log_branches", set()).add(("s" if a_ else "S") + ("n" if b_ else "t"))
    A = np.where(ss, np.where(near, one / F64(2), A_st), np.where(near, A_Ss, A_St))
    B = np.where(ss, np.where(near, one / F64(6), B_st), np.where(near, B_Ss, B_St))
    Cc = np.where(ss, one, C_S)
    zero = np.zeros_like(d)
    Om = [[zero, -o[2], o[1]], [o[2], zero, -o[0]], [-o[1], o[0], zero]]
    with np.errstate(all="ignore"):
        M = []
        for i in range(3):
            row = []
            for j in range(3):
                om2 = Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j]
                row.append((A * Om[i][j] + B * om2) + Cc * (one if i == j else F64(0)))
            row.append(S[4 + i])
            M.append(row)
    up = _solve3(M)
    return np.stack([o[0], o[1], o[2], up[0], up[1], up[2], sigma])


def _error(Cm, Si, Sj, trace=None):
    return sim3_log(_mul(_mul(Cm, Si), _inverse(Sj)), trace)


# ---------------------------------------------------------------------------------------------------------------- symbolic
def ordering(nv, edges, fixed):
    """The elimination order in rounds and the structure of L: per round the vertices still in the graph by ascending (current
    degree, vertex index), one taken when no neighbour has been taken in this round; eliminating it joins its neighbours.
    Returns (order [vertex], rounds [[position]], rows {position: sorted positions of the column's off-diagonal blocks})."""
    has = set()
    for i, j, _ in edges:
        has.add(int(i)); has.add(int(j))
    left = [v for v in range(nv) if not fixed[v] and v in has]
    adj = {v: set() for v in left}
    for i, j, _ in edges:
        i, j = int(i), int(j)
        if i in adj and j in adj:
            adj[i].add(j); adj[j].add(i)
    order, rounds, nbrs = [], [], {}
    while left:
        taken, blocked = [], set()
        for v in sorted(left, key=lambda v: (len(adj[v]), v)):
            if v in blocked:
                continue
            taken.append(v)
            blocked |= adj[v]
        rounds.append(list(range(len(order), len(order) + len(taken))))
        for v in taken:
            nb = adj.pop(v)
            nbrs[v] = set(nb)
            order.append(v)
            for a in nb:
                adj[a].discard(v)
                adj[a] |= nb - {a}
        left = [v for v in left if v in adj]
    pos = {v: k for k, v in enumerate(order)}
    rows = {pos[v]: sorted(pos[a] for a in nbrs[v]) for v in order}
    return order, rounds, rows


# ------------------------------------------------------------------------------------------------------------------ the run
def _seq(vals):
    s = F64(0)
    for v in vals:
        s = s + v
    return s


def _chains(vals):
    """64 interleaved chains, the partials added in order of the chain"""
    return _seq([_seq(vals[ch::CHAINS]) for ch in range(CHAINS)])


def _outer_k(A, B):
    """G[r][c] = sum_k A[r][k] B[c][k], k ascending"""
    G = A[:, 0][:, None] * B[:, 0][None, :]
    for k in range(1, 7):
        G = G + A[:, k][:, None] * B[:, k][None, :]
    return G


class State:
    pass


def _setup(p, trace):
    st = State()
    st.S0 = np.ascontiguousarray(p["Scw"], F64).reshape(-1, 8)
    st.nv = len(st.S0)
    st.fixed = np.asarray(p.get("fixed", np.zeros(st.nv, np.uint8))).astype(bool)
    nc = p.get("non_corrected")
    st.Snc = st.S0.copy()
    if nc is not None:
        has = np.asarray(p["has_non_corrected"]).astype(bool)
        st.Snc[has] = np.asarray(nc, F64).reshape(-1, 8)[has]
    st.edges = np.asarray(p.get("edges", np.zeros((0, 3), np.int32)), np.int64).reshape(-1, 3)
    st.ne = len(st.edges)
    st.fix_scale = bool(p.get("fix_scale", False))
    st.order, st.rounds, st.rows = ordering(st.nv, st.edges, st.fixed)
    st.pos = {v: k for k, v in enumerate(st.order)}
    st.nact = len(st.order)
    st.est = st.S0.T.copy()                                      # [8, nv]
    ei, ej, kind = st.edges[:, 0], st.edges[:, 1], st.edges[:, 2]
    st.ei, st.ej = ei, ej
    if st.ne:
        src_i = np.where(kind[None, :] == 1, st.S0.T[:, ei], st.Snc.T[:, ei])
        src_j = np.where(kind[None, :] == 1, st.S0.T[:, ej], st.Snc.T[:, ej])
        st.meas = _mul(src_j, _inverse(src_i))
    act = np.zeros(st.nv, bool)
    act[st.order] = True
    st.vact = act
    st.eact = (act[ei] | act[ej]) if st.ne else np.zeros(0, bool)
    st.inc = {c: [] for c in range(st.nact)}                    # incident (edge, side) by column, ascending edge index
    st.offd = {}                                                 # (row, column) -> [(edge, side of the row vertex)]
    for e in range(st.ne):
        for side, v in enumerate((int(ei[e]), int(ej[e]))):
            if act[v]:
                st.inc[st.pos[v]].append((e, side))
        if act[ei[e]] and act[ej[e]]:
            ci, cj = st.pos[int(ei[e])], st.pos[int(ej[e])]
            st.offd.setdefault((max(ci, cj), min(ci, cj)), []).append((e, 0 if ci > cj else 1))
    st.trace = trace
    return st


def _errors(st):
    """computeActiveErrors: err [7, ne] (zero on an inactive edge) and the chi2 per edge"""
    if not st.ne:
        return np.zeros((7, 0)), np.zeros(0)
    err = _error(st.meas, st.est[:, st.ei], st.est[:, st.ej], st.trace)
    err = np.where(st.eact[None, :], err, F64(0))
    chi = err[0] * err[0]
    for k in range(1, 7):
        chi = chi + err[k] * err[k]
    return err, chi


def _system(st):
    err, chi = _errors(st)
    scalar = F64(1) / (F64(2) * DELTA)
    J = np.zeros((2, 7, 7, st.ne))                               # side, column d, component k
    Si, Sj = st.est[:, st.ei], st.est[:, st.ej]
    for side in range(2):
        for d in range(7):
            ev = []
            for sign in (DELTA, -DELTA):
                u = np.zeros((7, st.ne))
                u[d] = sign
                P = _oplus(Sj if side else Si, u, st.fix_scale)
                ev.append(_error(st.meas, Si, P) if side else _error(st.meas, P, Sj))
            J[side, d] = scalar * (ev[0] - ev[1])
    Je = np.transpose(J, (3, 0, 1, 2))                           # [e][side][d][k]
    A, b = {}, np.zeros((st.nact, 7))
    for c in range(st.nact):
        acc, bb = np.zeros((7, 7)), np.zeros(7)
        for ch in range(CHAINS):
            pa, pb = np.zeros((7, 7)), np.zeros(7)
            for e, side in st.inc[c][ch::CHAINS]:
                Jv = Je[e, side]
                pa = pa + _outer_k(Jv, Jv)
                g = Jv[:, 0] * err[0, e]
                for k in range(1, 7):
                    g = g + Jv[:, k] * err[k, e]
                pb = pb - g
            acc, bb = acc + pa, bb + pb
        A[(c, c)], b[c] = acc, bb
    for key, ent in st.offd.items():
        acc = np.zeros((7, 7))
        for e, side in ent:
            acc = acc + _outer_k(Je[e, side], Je[e, 1 - side])
        A[key] = acc
    return A, b, _chains(list(chi))


def _ldl7(M):
    """the unpivoted 7 x 7 L D L^T in place (lower triangle): returns d"""
    d = np.zeros(7)
    for j in range(7):
        s = M[j, j]
        for k in range(j):
            s = s - M[j, k] * (M[j, k] * d[k])
        d[j] = s
        for i in range(j + 1, 7):
            t = M[i, j]
            for k in range(j):
                t = t - M[i, k] * (M[j, k] * d[k])
            M[i, j] = t / s
    return d


def block_solve(st, A, b, lam):
    """(H + lambda I) x = b by the block L D L^T round by round; (ok, x [nact, 7])"""
    L, D = {}, {}
    below = {c: [] for c in range(st.nact)}                     # row -> its columns, ascending
    with np.errstate(all="ignore"):
        for cols in st.rounds:
            for j in cols:
                for i in [j] + st.rows[j]:
                    T = A.get((i, j), np.zeros((7, 7))).copy()
                    if i == j:
                        for r in range(7):
                            T[r, r] = T[r, r] + lam
                    for k in below[i]:
                        if k >= j or (j, k) not in L:
                            continue
                        W = L[(i, k)] * D[k][None, :]
                        T = T - _outer_k(W, L[(j, k)])
                    L[(i, j)] = T
            for j in cols:
                D[j] = _ldl7(L[(j, j)])
            for j in cols:
                Ljj, d = L[(j, j)], D[j]
                for i in st.rows[j]:
                    Tm = L[(i, j)]
                    for c in range(7):
                        t = Tm[:, c]
                        for m in range(c):
                            t = t - (Tm[:, m] * d[m]) * Ljj[c, m]
                        Tm[:, c] = t / d[c]
                    below[i].append(j)
        x = np.zeros((st.nact, 7))
        ok = all(bool((D[j] > 0).all() and (D[j] <= DBL_MAX).all()) for j in range(st.nact))
        if not ok:
            return False, x, L, D
        y = np.zeros((st.nact, 7))
        for cols in st.rounds:
            for j in cols:
                v = b[j].copy()
                for k in below[j]:
                    Lk = L[(j, k)]
                    s = Lk[:, 0] * y[k][0]
                    for m in range(1, 7):
                        s = s + Lk[:, m] * y[k][m]
                    v = v - s
                Ljj = L[(j, j)]
                for r in range(1, 7):
                    for m in range(r):
                        v[r] = v[r] - Ljj[r, m] * v[m]
                y[j] = v
        for cols in reversed(st.rounds):
            for j in cols:
                v = y[j] / D[j]
                for i in st.rows[j]:
                    Li = L[(i, j)]
                    s = Li[0, :] * x[i][0]
                    for r in range(1, 7):
                        s = s + Li[r, :] * x[i][r]
                    v = v - s
                Ljj = L[(j, j)]
                for c in range(5, -1, -1):
                    for m in range(c + 1, 7):
                        v[c] = v[c] - Ljj[m, c] * v[m]
                x[j] = v
    return True, x, L, D


def _canon64(v):
    a = np.array(v, F64)
    u = a.view(np.uint64)
    u[np.isnan(a)] = CANON64
    return a


def _canon32(v):
    a = np.array(v, np.float32)
    u = a.view(np.uint32)
    u[np.isnan(a)] = CANON32
    return a


def run(p, trace=None):
    """One problem (the dict optimizer.optimize_essential_graph_batch takes) -> dict: Siw [nv, 8] float64, Tiw [nv, 16] float32,
    world [npoints, 3] float32, iters, nactive, nfailed, nrounds, nlblocks, chi2 [2], lambda"""
    st = _setup(p, trace)
    out = dict(iters=0, nactive=st.nact, nfailed=0, nrounds=len(st.rounds), nlblocks=st.nact + sum(len(r) for r in st.rows.values()))
    chi2, lam = [F64(0), F64(0)], F64(0)
    with np.errstate(all="ignore"):
        if st.nact:
            it, nu, stall, cur = 0, F64(2), 0, F64(0)
            verts = np.array(st.order)
            while it < ITERS:
                A, b, cur = _system(st)
                ini = cur
                if it == 0:
                    chi2[0] = cur
                    lam, nu, stall = LAMBDA0, F64(2), 0
                it += 1
                rho, q = F64(0), 0
                while True:
                    ok, x, _, _ = block_solve(st, A, b, lam)
                    if not ok:
                        out["nfailed"] += 1
                    bak = st.est.copy()
                    u = x.T.copy()
                    st.est[:, verts] = _oplus(st.est[:, verts], u, st.fix_scale)
                    x = u.T.copy()                               # (x[6] zeroed in place under fix_scale)
                    tmp = _chains(list(_errors(st)[1]))
                    if not ok:
                        tmp = DBL_MAX
                    rho = cur - tmp
                    sc = []
                    for col in range(st.nact):
                        sc.append((col, x[col], b[col]))
                    parts = []
                    for ch in range(CHAINS):
                        s = F64(0)
                        for col, xv, bv in sc[ch::CHAINS]:
                            for j in range(7):
                                s = s + xv[j] * (lam * xv[j] + bv[j])
                        parts.append(s)
                    scale = _seq(parts) + F64(1e-3)
                    rho = rho / scale
                    if rho > 0 and np.abs(tmp) <= DBL_MAX:
                        r2 = F64(2) * rho - F64(1)
                        alpha = F64(1) - (r2 * r2) * r2
                        alpha = F64(2) / F64(3) if F64(2) / F64(3) < alpha else alpha
                        sf = alpha if F64(1) / F64(3) < alpha else F64(1) / F64(3)
                        lam = lam * sf
                        nu = F64(2)
                        cur = tmp
                    else:
                        lam = lam * nu
                        nu = nu * F64(2)
                        st.est = bak
                    q += 1
                    if not (rho < 0 and q < TRIALS):
                        break
                if q == TRIALS or rho == 0:
                    break
                stall = stall + 1 if (ini - cur) * F64(1e3) < ini else 0
                if stall >= 3:
                    break
            out["iters"] = it
            chi2[1] = cur
        S = st.est
        R = _R_from_quat(S)
        inv_s = F64(1) / S[7]
        T = np.zeros((st.nv, 16), np.float32)
        for r in range(3):
            for c in range(3):
                T[:, 4 * r + c] = R[r][c].astype(np.float32)
            T[:, 4 * r + 3] = (S[4 + r] * inv_s).astype(np.float32)
        T[:, 15] = 1
        out["Siw"] = _canon64(S.T)
        out["Tiw"] = _canon32(T)
        world = np.ascontiguousarray(p.get("world", np.zeros((0, 3), np.float32)), np.float32).reshape(-1, 3)
        ref = np.asarray(p.get("ref", np.zeros(0, np.int32)), np.int64).reshape(-1)
        wout = world.copy()
        live = ref >= 0
        if live.any():
            r = ref[live]
            Srw = st.S0.T[:, r]
            Swr = _inverse(out["Siw"].T[:, r])
            w = world[live].astype(F64)
            a = _rotate(Srw, w[:, 0], w[:, 1], w[:, 2])
            a = [Srw[7] * a[k] + Srw[4 + k] for k in range(3)]
            g = _rotate(Swr, a[0], a[1], a[2])
            wout[live] = _canon32(np.stack([Swr[7] * g[k] + Swr[4 + k] for k in range(3)], axis=1).astype(np.float32))
        out["world"] = wout
    out["chi2"] = _canon64(chi2)
    out["lambda"] = _canon64([lam])[0]
    return out


def dense_system(p, lam):
    """tests: the assembled dense H + lambda I and b of the first linearisation, in elimination order, and the block solution"""
    st = _setup(p, None)
    A, b, _ = _system(st)
    n = 7 * st.nact
    H = np.zeros((n, n))
    for (i, j), blk in A.items():
        H[7 * i:7 * i + 7, 7 * j:7 * j + 7] = blk
        if i != j:
            H[7 * j:7 * j + 7, 7 * i:7 * i + 7] = blk.T
    H = H + lam * np.eye(n)
    ok, x, _, _ = block_solve(st, A, b, F64(lam))
    return H, b.reshape(-1), ok, x.reshape(-1)
