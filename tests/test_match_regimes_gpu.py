"""The size-selected launch regimes of the brute-force matcher (orbx_launch_match, rule in csrc/orbx_launch.h), each with planted
edges and compared with oracle.match_bruteforce pair by pair, exactly:

  matrix-pipe kernels (k_match_f4 = default, k_match = ORBX_MATCH_KERNEL=i8), waves4 = ceil(out_stride / 128) * npairs
    waves4 >= 2048  QT = 4, no train split, direct output
    otherwise       QT = 2, nsplit = min(16, max(1, 4096 / (ceil(out_stride / 64) * npairs))), k_match_merge when nsplit > 1
  vector-pipe kernel (k_match_valu): nsplit = min(16, max(1, ceil(16384 / (ceil(out_stride / 128) * npairs)))), always merged

Small calls (everything tests/test_gpu_parity.py launches) are nsplit = 16; the cases here are the smallest launches that reach
QT = 4, the direct-output branch of QT = 2, the splits 2, 3 and 7 (split boundaries inside the train set, empty shares), the
loop over key tables of 4096 train rows (without a split, and inside a split launch), nsplit 1 and 4 of the vector-pipe kernel,
and the last train index the result packing holds (2^20 - 1).  Every case first asserts through orbx_debug_match_plan that it
is in the regime it is meant for: a changed heuristic fails there instead of silently testing another regime.

Data: one descriptor pool per side on the device, shared by all pairs through overlapping strides (q_stride = 32 bytes: pair p's
queries start at pool row p; t_stride = 64: its train rows at pool row 2 p), so a few hundred KB serve thousands of pairs and the
planted rows land at different tile, split and chunk positions in different pairs."""
import ctypes as C
import functools
import numpy as np
import pytest
import oracle
from orb_slam2_detailed_comments_amd import ORBextractor, ORBmatcher, _capi

Q_STRIDE, T_STRIDE = 32, 64      # bytes; multiples of 32 keep the kernels' 16-byte loads aligned
PREFILL = -7
NONE = 0x7fffffff                # best / second distance of "no such train row"
# name: (npairs, out_stride, (qt, nsplit))
MFMA_CASES = {
    "qt4_direct": (2048, 128, (4, 1)),          # QT = 4 with planted edges; the chunk loop
    "qt2_direct": (2047, 100, (2, 1)),          # the direct-output branch of QT = 2; the chunk loop
    "split3": (1365, 64, (2, 3)),               # an intermediate split
    "split7": (585, 64, (2, 7)),                # an intermediate split with empty shares
    "split2_chunks": (2047, 64, (2, 2)),        # the chunk loop inside a split launch
}
VALU_CASES = {"nsplit1": (16384, 8, (0, 1)), "nsplit4": (5000, 8, (0, 4))}
ENV = {"mfma_fp4": None, "mfma_i8": "i8", "valu": "valu"}     # ORBX_MATCH_KERNEL, read once per handle
LIMIT = 1 << 20                  # train rows per pair (include/orbx.h): the index is packed into 20 bits below the distance


def match_plan(handle, npairs, out_stride):
    qt, nsplit = C.c_int(-1), C.c_int(-1)
    _capi.check(_capi.lib().orbx_debug_match_plan(handle, npairs, out_stride, C.byref(qt), C.byref(nsplit)))
    return qt.value, nsplit.value


def _flip(row, nbits):
    out = row.copy()
    for b in range(nbits):
        out[b] ^= 1
    return out


def _counts(rng, npairs, special_q, special_t, q_max, t_max):
    """every (special nq, special nt) combination in the first pairs, random counts behind them"""
    nq = rng.integers(0, q_max + 1, npairs).astype(np.int32)
    nt = rng.integers(0, t_max + 1, npairs).astype(np.int32)
    ncomb = len(special_q) * len(special_t)
    assert ncomb < npairs
    p = np.arange(ncomb)
    nq[:ncomb] = np.asarray(special_q)[p % len(special_q)]
    nt[:ncomb] = np.asarray(special_t)[p // len(special_q)]
    return nq, nt, ncomb


@functools.lru_cache(maxsize=None)
def build_case(name):
    """pools, counts and the oracle's answer for every pair of one case (computed once, shared by the kernels; never modified)"""
    valu = name in VALU_CASES
    npairs, stride, _ = (VALU_CASES if valu else MFMA_CASES)[name]
    rng = np.random.default_rng(sorted(list(MFMA_CASES) + list(VALU_CASES)).index(name) + 100)
    beyond = stride + 72                                     # a count beyond out_stride: ignored, nothing written for it
    if valu:
        nq, nt, ncomb = _counts(rng, npairs, [0, 1, 7, 8, beyond], [0, 1, 2, 31, 32, 33, 40], stride, 40)
    elif stride == 64:                                       # the split launches
        nq, nt, ncomb = _counts(rng, npairs, [0, 1, 31, 32, 33, 63, 64, beyond], [0, 1, 33, 95, 96, 97, 129], stride, 300)
    else:
        nq, nt, ncomb = _counts(rng, npairs, [0, 1, 31, 32, 33, stride - 1, stride, beyond], [0, 1, 31, 32, 33], stride, 300)
    # pairs with more train rows than one key table (4096), ten pairs apart at the end of the list: their windows reach past
    # every other pair's.  (train rows, query count)
    large = {"qt4_direct": [(4096, 128), (4097, 33), (8192, beyond), (8200, 127)],
             "qt2_direct": [(4096, 100), (4097, 33), (8192, beyond), (8200, 99)],
             "split2_chunks": [(8300, 64)]}.get(name, [])
    large_at = [npairs - 1 - 10 * k for k in range(len(large))]
    for p, (n_t, n_q) in zip(large_at, large):
        nt[p], nq[p] = n_t, n_q
    assert min(large_at, default=npairs) >= ncomb
    q_rows = npairs + beyond
    t_rows = 2 * npairs + int(nt.max()) + 64
    q = rng.integers(0, 256, (q_rows, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (t_rows, 32), dtype=np.uint8)
    # ---- planted everywhere (a pair sees them at an offset that depends on p)
    t[17::101] = 0; t[18::101] = 255                         # popcounts 0 and 256
    q[7::53] = 0; q[8::53] = 255                             # ... distances 0 and 256 against them
    k = np.arange(3, min(q_rows, (t_rows - 20) // 2), 5 if valu else 29)
    t[2 * k + 17] = t[2 * k + 6]                             # equal train rows 11 apart: the first index wins, second == best
    q[k] = t[2 * k + 6]                                      # in pair p = k - i, query i equals train rows 2 i + 6 and 2 i + 17
    # ---- planted for one pair each; `expect` = (pair, query, best index, best distance, second distance) the oracle must return
    expect = []
    free = [p for p in range(ncomb + 100, npairs - 200) if nt[p] >= 35 and nq[p] >= 4]
    for p in (free[0], [p for p in free if p >= free[0] + 160][0]):   # (far enough apart that their windows do not meet)
        n_t = int(nt[p])
        t[2 * p:2 * p + n_t] = rng.integers(0, 256, (n_t, 32), dtype=np.uint8)   # a window with nothing else in it
        q[p + 1] = t[2 * p + n_t - 1]                        # query 1 = the last train row
        expect.append((p, 1, n_t - 1, 0, None))
        t[2 * p + 3] = 255; t[2 * p + 33] = 255; q[p + 2] = 255   # equal rows in two tiles, popcount 256
        expect.append((p, 2, 3, 0, 0))
    p = [p for p in range(ncomb) if nt[p] == 1 and nq[p] >= 1][0]
    t[2 * p] = 255; q[p] = 0                                 # the only train row at distance 256
    expect.append((p, 0, 0, 256, NONE))
    if not valu:
        p = [p for p in range(ncomb) if nt[p] == 33 and nq[p] >= 32][0]
        q[p + 31] = t[2 * p + 32]                            # the one row of the second tile (the second split's whole share)
        expect.append((p, 31, 32, 0, None))
    for p, (n_t, n_q) in zip(large_at, large):
        b = 2 * p
        if name == "split2_chunks":                          # per = 4160 rows per split: chunks [0, 4096) [4096, 4160) | [4160, 8256) [8256, 8300)
            plants = [(0, [(5, 0), (4101, 0)]),              # tied across the key-table boundary inside split 0
                      (1, [(n_t - 1, 0)]),                   # the last train row: the last chunk of the last split
                      (2, [(4159, 0), (4160, 0)]),           # tied across the split boundary
                      (3, [(8259, 0), (4162, 1)])]           # best in a split's second chunk, second-best in its first
        else:
            plants = [(0, [(5, 0)] + ([(4101, 0)] if n_t > 4101 else [])),   # tied across the key-table boundary
                      (1, [(n_t - 1, 0)]),                                   # best in the last chunk: the last train row
                      (2, [(4095 if n_t > 4096 else 4064, 0)])]              # best in the first chunk, at its last row / last tile
            if n_t > 4103:
                plants.append((3, [(4103, 0), (9, 1)]))      # best in a later chunk, second-best (one bit off) in the first
        for qi, rows in plants:
            for row, bits in rows:
                t[b + row] = _flip(q[p + qi], bits)
            d = sorted((bits, row) for row, bits in rows)
            expect.append((p, qi, d[0][1], d[0][0], d[1][0] if len(d) > 1 else None))
    # ---- the oracle, pair by pair; nothing is left out
    exp = [np.full((npairs, stride), PREFILL, np.int32) for _ in range(3)]
    for p in range(npairs):
        n = min(int(nq[p]), stride)
        if n:
            for e, o in zip(exp, oracle.match_bruteforce(q[p:p + n], t[2 * p:2 * p + int(nt[p])])):
                e[p, :n] = o
    # ---- the planted cases are there (a test that plants nothing passes for nothing)
    for p, qi, idx, best, second in expect:
        assert qi < min(nq[p], stride) and (exp[0][p, qi], exp[1][p, qi]) == (idx, best), (name, p, qi, exp[0][p, qi], exp[1][p, qi])
        assert second is None or exp[2][p, qi] == second, (name, p, qi, exp[2][p, qi])
    live = exp[0] != PREFILL
    assert ((exp[1] == 0) & (exp[2] == 0) & live).sum() >= 8, "ties of equal train rows"
    assert ((exp[0] == -1) & live).any() and (exp[1][live] == NONE).any(), "queries without train rows"
    assert (exp[2][live] == NONE).sum() > (exp[1][live] == NONE).sum(), "a single train row"
    assert (nq > stride).any() and (nq == 0).any() and ((nq > 0) & (nt == 0)).any()
    for a in (q, t, nq, nt, *exp):
        a.setflags(write=False)
    return dict(npairs=npairs, stride=stride, q=q, t=t, nq=nq, nt=nt, exp=exp)


def test_case_shapes_and_plants():
    """CPU part: every case builds, holds its planted rows (asserted inside build_case against the oracle) and stays inside its
    pools; the share arithmetic of the kernels gives the intended empty shares and chunk counts"""
    for name in list(MFMA_CASES) + list(VALU_CASES):
        c = build_case(name)
        p = np.arange(c["npairs"])
        assert (p + np.minimum(c["nq"], c["stride"]) <= len(c["q"])).all() and (2 * p + c["nt"] <= len(c["t"])).all()
    for name, nsplit in (("split3", 3), ("split7", 7)):
        nt = build_case(name)["nt"]
        per = ((nt + 31) // 32 + nsplit - 1) // nsplit * 32          # k_match: a block's share, in whole tiles of 32
        assert ((nt > 0) & ((nsplit - 1) * per >= nt)).any(), "no pair whose last split gets an empty share"
        assert ((nt % 32 != 0) & (per < nt) & (nt % np.maximum(per, 1) != 0)).any(), "no split boundary inside a ragged train set"
    nt = int(build_case("split2_chunks")["nt"].max())
    assert ((nt + 31) // 32 + 1) // 2 * 32 > 4096, "the split share does not exceed one key table"
    assert sorted(build_case("qt4_direct")["nt"][-31::10]) == [4096, 4097, 8192, 8200]


def _run_case(kernel, name, expected_plan, monkeypatch):
    import torch
    if ENV[kernel]:
        monkeypatch.setenv("ORBX_MATCH_KERNEL", ENV[kernel])
    else:
        monkeypatch.delenv("ORBX_MATCH_KERNEL", raising=False)
    c = build_case(name)
    npairs, stride = c["npairs"], c["stride"]
    ex = ORBextractor(300)
    plan = match_plan(ex.handle, npairs, stride)
    assert plan == expected_plan, f"{kernel} {name}: {npairs} pairs x out_stride {stride} launch as (qt, nsplit) = {plan}, the case is meant for {expected_plan}"
    dev = torch.device("cuda", 0)
    dq, dt = torch.from_numpy(c["q"].copy()).to(dev), torch.from_numpy(c["t"].copy()).to(dev)
    dnq, dnt = torch.from_numpy(c["nq"].copy()).to(dev), torch.from_numpy(c["nt"].copy()).to(dev)
    out = [torch.full((npairs, stride), PREFILL, dtype=torch.int32, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    _capi.check(_capi.lib().orbx_match_bruteforce_device(ex.handle, npairs, _capi.ptr(dq), _capi.ptr(dnq), Q_STRIDE, _capi.ptr(dt), _capi.ptr(dnt),
                                                         T_STRIDE, _capi.ptr(out[0]), _capi.ptr(out[1]), _capi.ptr(out[2]), stride))
    ex.synchronize()
    got = [o.cpu().numpy() for o in out]
    ex.close()
    for g, e, what in zip(got, c["exp"], ("best index", "best distance", "second distance")):
        if not np.array_equal(g, e):       # (outputs beyond min(nq, out_stride) are the prefill in `e`)
            p, qi = np.argwhere(g != e)[0]
            raise AssertionError(f"{kernel} {name} plan {plan}: {what} of pair {p} (nq {c['nq'][p]}, nt {c['nt'][p]}) query {qi}: "
                                 f"{g[p, qi]}, oracle {e[p, qi]}; {int((g != e).sum())} entries differ")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MFMA_CASES))
@pytest.mark.parametrize("kernel", ["mfma_fp4", "mfma_i8"])
def test_matrix_pipe_regimes_equal_the_oracle(kernel, name, monkeypatch):
    _run_case(kernel, name, MFMA_CASES[name][2], monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VALU_CASES))
def test_vector_pipe_splits_equal_the_oracle(name, monkeypatch):
    _run_case("valu", name, VALU_CASES[name][2], monkeypatch)


@functools.lru_cache(maxsize=None)
def limit_case():
    rng = np.random.default_rng(20)
    q = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (LIMIT + 40, 32), dtype=np.uint8)
    t[LIMIT - 1] = q[0]          # the best match of query 0 at the last index the packing holds
    t[LIMIT + 7] = q[1]          # an exact copy of query 1 beyond the limit only
    exp = oracle.match_bruteforce(q, t[:LIMIT])
    full = oracle.match_bruteforce(q, t)
    assert (exp[0][0], exp[1][0]) == (LIMIT - 1, 0) and exp[2][0] > 0
    assert (full[0][1], full[1][1]) == (LIMIT + 7, 0) and exp[1][1] > 0 and exp[0][1] < LIMIT
    for a in (q, t, *exp):
        a.setflags(write=False)
    return q, t, exp


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", list(ENV))
def test_train_rows_up_to_the_packing_limit(kernel, monkeypatch):
    """one pair, nq = 3, nt = 2^20 + 40 in the default regime of a small call (nsplit = 16; 2^16 rows = 16 key tables per split
    on the matrix pipe): the result equals the oracle on the first 2^20 rows -- index 2^20 - 1 survives the packing, rows beyond
    the limit are ignored as include/orbx.h says"""
    if ENV[kernel]:
        monkeypatch.setenv("ORBX_MATCH_KERNEL", ENV[kernel])
    else:
        monkeypatch.delenv("ORBX_MATCH_KERNEL", raising=False)
    q, t, exp = limit_case()
    ex = ORBextractor(300)
    plan = match_plan(ex.handle, 1, len(q))
    assert plan == ((0, 16) if kernel == "valu" else (2, 16)), f"{kernel}: a single small pair launches as {plan}, not in the default regime"
    got = ORBmatcher(0.9, True, extractor=ex).match_bruteforce(q, t)
    ex.close()
    for g, e, what in zip(got, exp, ("best index", "best distance", "second distance")):
        assert np.array_equal(g, e), f"{kernel} plan {plan}: {what} {g}, oracle on the first 2^20 rows {e}"
