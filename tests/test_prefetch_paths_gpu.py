"""The hand-over between two tiles in the kernels that prefetch one: k_fast_rows / k_fast_rows_ip / k_fast_rows_l0 with two
groups per wave (the second group's tile is requested into a register set of its own while the first group is processed), and
the tile loop of k_match_f4 / k_match (the next train tile is requested before the MFMAs of the current one; rows past the
pair's count must read as zero whatever the buffer holds there -- by a predicated load as the kernels stand, by a clamped row and
selects in the form profiles/prefetch_waits.md measured).
tests/test_fast_net_gpu.py, tests/test_fast_first_plan.py and tests/test_match_regimes_gpu.py cover the common paths; this file
adds what a broken hand-over would get wrong.

FAST: ORBX_FAST_GPW=2 against ORBX_FAST_GPW=1 byte for byte (keypoint records, descriptors, counts: keys, order and counts) and
against the oracle, on the slab, in-place mixed and FAST-first paths, eight planted frames per case, on three geometries chosen
with the launcher's group model (test_fast_net_gpu.fast_groups, restated here with scale and level count) so that
  (a) a launch has an odd group count: its last wave has one group;
  (b) in the mixed kernel a wave pairs a level-0 in-place group with a slab group.  Levels ascend in every launch, so the in-place
      group is always the wave's first: the other order does not exist (asserted below), whatever the geometry;
  (c) a reflected first cell row is paired with an interior one, and an interior one with the reflected last row;
  (d) a wave's second group, and another wave's first, has cells taller than the 45 register rows: the extra rows are loaded
      behind a prefetched tile;
  (e) a wave's first group passes more candidates than the work list holds, so its walk is chunked, with the second tile's loads
      outstanding across the flushes.
Every run asserts through orbx_debug_fast_gpw that its launches took the groups per wave it forced.

Matcher: FP4 and ORBX_MATCH_KERNEL=i8 against a numpy brute force (best index, best distance, second distance), train counts
0, 1, 31, 32, 33, 63, 64, 65 x query counts 1, 33, 128 in the first pairs of every launch, other counts behind them, once with
a few pairs (QT = 2; with 4096 and 4097 train rows among them) and with 2048 pairs (QT = 4; the last pair has 4096 or 4097 train
rows, the boundary of the key table, unsplit), the regime asserted through orbx_debug_match_plan.  Every pair has its own rows in
the device buffers, with slack behind them, and every row past nq / nt is 0xFF bytes; the first and the last query of each pair
are all ones but three bits, so a garbage row that leaked into the result would be their best match by far."""
import ctypes as C
import functools
import numpy as np
import pytest
import oracle
import upstream_model
from orb_slam2_detailed_comments_amd import ORBextractor, _capi
import test_fast_net_gpu as fast
import test_match_regimes_gpu as regimes

# ------------------------------------------------------------------------------------------------ FAST
NFEAT, PAIR, LCAP = 300, (20, 7), 640
GEOMS = {"odd128": (128, 96, 1.2, 8), "rows152": (152, 136, 1.2, 8), "coarse140": (140, 100, 2.0, 3)}   # w, h, scale, levels
FRAME_IDS = [0, 1, 8, 10, 11, 12, 14, 15]      # of test_fast_net_gpu.planted_frames: dots, blocks, stripes, noise, synthetic
CASES = [("odd128", None), ("odd128", "64"), ("rows152", None), ("coarse140", None)]     # geometry, ORBX_FAST_LCAP


def groups(geom):
    """test_fast_net_gpu.fast_groups for a geometry of GEOMS: (level, [cells (x0, y0, cw, ch)]) in launch order"""
    w, h, scale, nlevels = GEOMS[geom]
    out = []
    for l, g in enumerate(upstream_model.geometry(w, h, NFEAT, scale, nlevels, padded=True)):
        cells = [c[:4] for c in g["cells"] if c[2] >= 7 and c[3] >= 7]
        i = 0
        while i < len(cells):
            n = 1
            if i + 1 < len(cells):
                a, b = cells[i], cells[i + 1]
                if b[1] == a[1] and b[3] == a[3] and b[0] == a[0] + a[2] - 6 and (a[2] - 6) + (b[2] - 6) <= 64 + 2:
                    n = 2
            out.append((l, cells[i:i + n]))
            i += n
    return out


def launches(path, nframes, geom):
    """(frames, first group, groups) of every FAST launch of one batch call"""
    g = groups(geom)
    l0, total = sum(1 for l, _ in g if l == 0), len(g)
    if path != "fastfirst":
        return [(nframes, 0, total)]
    return [(nframes, 0, l0)] + [(b, l0, total - l0) for b in fast.split_batch(nframes, 3)]


def waves(geom, first, count):
    """the groups of each wave of a launch over groups [first, first + count) at two groups per wave"""
    g = groups(geom)[first:first + count]
    return [g[i:i + 2] for i in range(0, len(g), 2)]


def row_kind(geom, cells):
    """level-0 in place: the first and the last cell row read reflected source rows (csrc/orbx_inplace.h, ORBX_EDGE = 19)"""
    h = GEOMS[geom][1]
    y0, ch = cells[0][1], cells[0][3]
    return "first" if y0 < 19 else "last" if y0 + ch - 1 - 19 >= h else "interior"


@functools.lru_cache(maxsize=None)
def frames_and_oracle(geom):
    w, h, scale, nlevels = GEOMS[geom]
    frames = np.ascontiguousarray(fast.planted_frames(w, h)[FRAME_IDS])
    orc = oracle.OracleExtractor(NFEAT, scale, nlevels, *PAIR)
    ref = [orc.extract(f)[:2] for f in frames]
    frames.setflags(write=False)
    return frames, ref


def test_geometries_hold_the_pairings():
    """CPU part: the geometries and frames give every pairing (a) - (e) of the docstring"""
    n = len(FRAME_IDS)
    found = set()
    for geom in GEOMS:
        for path in fast.PATHS:
            for b, first, count in launches(path, n, geom):
                wv = waves(geom, first, count)
                assert len(wv) == -(-count // 2) and all(len(x) == 2 for x in wv[:-1])
                if count % 2:
                    assert len(wv[-1]) == 1
                    found.add(("a", path))
                for x in wv:
                    if len(x) < 2:
                        continue
                    (la, ca), (lb, cb) = x
                    assert la <= lb, "levels ascend in every launch: a slab group never precedes an in-place one in a wave"
                    if path == "inplace" and la == 0 and lb > 0:
                        found.add("b")
                    if path != "slab" and la == 0 and lb == 0:
                        found.add(("c", row_kind(geom, ca), row_kind(geom, cb)))
                    if lb > 0 and cb[0][3] > 45:
                        found.add(("d2", path))
                    if la > 0 and ca[0][3] > 45:
                        found.add(("d1", path))
    assert {("a", p) for p in fast.PATHS} <= found and "b" in found
    assert ("c", "first", "interior") in found and ("c", "interior", "last") in found
    assert {(d, p) for d in ("d1", "d2") for p in fast.PATHS} <= found
    # (e) candidates of the walk's pre-test (test_fast_net_gpu.margins) in the first group of a level-0 wave, per geometry
    for geom in GEOMS:
        frames, _ = frames_and_oracle(geom)
        l0 = [x for x in waves(geom, 0, len(groups(geom))) if len(x) == 2 and x[0][0] == 0 and x[1][0] == 0]
        full = False
        for f in frames:
            a = fast.margins(np.pad(f, 19, mode="reflect"))
            pre = np.maximum(a[2], a[3]) > PAIR[0]
            for (_, ca), _ in l0:
                x0, y0, ch = ca[0][0], ca[0][1], ca[0][3]
                ncol = min(ca[-1][0] + ca[-1][2] - 6 - x0, 64)
                full |= int(pre[y0:y0 + ch - 6, x0:x0 + ncol].sum()) > LCAP
        assert full, f"{geom}: no wave whose first group passes more than {LCAP} candidates"


def _run_fast(monkeypatch, path, geom, gpw, lcap):
    """one device call over the geometry's frames under the path's knobs; asserts the groups per wave of every FAST launch and
    returns (keypoint bytes, descriptor bytes, counts) as numpy arrays"""
    import torch
    w, h, scale, nlevels = GEOMS[geom]
    frames, _ = frames_and_oracle(geom)
    for k in fast.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in fast.PATHS[path].items():
        monkeypatch.setenv(k, v)
    if lcap:
        monkeypatch.setenv("ORBX_FAST_LCAP", lcap)
    monkeypatch.setenv("ORBX_FAST_GPW", gpw)
    n = len(frames)
    ex = ORBextractor(NFEAT, scale, nlevels, PAIR[0], PAIR[1], max_batch=n)
    ex.profile_enable(1 << _capi.K_NAMES.index("k_fast_rows"))
    cap = ex.max_keypoints(w, h)
    dev = torch.device("cuda", 0)
    imgs = torch.from_numpy(frames.copy()).to(dev)
    kps = torch.zeros((n, cap * 28), dtype=torch.uint8, device=dev)
    desc = torch.zeros((n, cap * 32), dtype=torch.uint8, device=dev)
    cnt = torch.full((n,), -3, dtype=torch.int32, device=dev)
    st = torch.full((n,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ex.extract_batch_device(imgs, n, w, h, imgs.stride(1), imgs.stride(0), kps, desc, cnt, st, cap)
    ex.synchronize()
    nlaunch = ex.profile_read()["k_fast_rows"][1]
    l0, total = C.c_int(0), C.c_int(0)
    _capi.check(_capi.lib().orbx_debug_fast_groups(ex.handle, C.byref(l0), C.byref(total)))
    g = groups(geom)
    assert (l0.value, total.value) == (sum(1 for l, _ in g if l == 0), len(g)), "the group model of this file is not the library's geometry"
    plan = launches(path, n, geom)
    took = [fast.fast_gpw(ex, b, count) for b, _, count in plan]
    assert not st.cpu().numpy().any()
    ex.close()
    assert nlaunch == len(plan), f"{path} {geom}: {nlaunch} FAST launches, modelled {plan}"
    assert took == [int(gpw)] * len(plan), f"{path} {geom} ORBX_FAST_GPW={gpw}: the launches run {took} groups per wave"
    return kps.cpu().numpy(), desc.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("geom,lcap", CASES, ids=[f"{g}-lcap{l}" for g, l in CASES])
@pytest.mark.parametrize("path", list(fast.PATHS))
def test_two_groups_per_wave_equal_one_and_the_oracle(path, geom, lcap, monkeypatch):
    _, ref = frames_and_oracle(geom)
    one = _run_fast(monkeypatch, path, geom, "1", lcap)
    two = _run_fast(monkeypatch, path, geom, "2", lcap)
    for a, b, what in zip(one, two, ("keypoint records", "descriptors", "counts")):
        assert a.tobytes() == b.tobytes(), f"{path} {geom} lcap {lcap}: {what} differ between one and two groups per wave"
    fast._assert_oracle(two[2], two[0].view(_capi.KP_DTYPE), ref, f"{path} {geom} lcap {lcap} gpw 2")


# ------------------------------------------------------------------------------------------------ matcher
NQS, NTS = (1, 33, 128), (0, 1, 31, 32, 33, 63, 64, 65)
STRIDE = 128                         # out_stride = max_nq
Q_ROWS = STRIDE + 5                  # rows per pair in the query buffer: five rows of slack
T_SLACK = 7
POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)
MATCH_CASES = {"qt2_few": (30, (2, 16)), "qt4_4096": (2048, (4, 1)), "qt4_4097": (2048, (4, 1))}   # pairs, (qt, nsplit)


def brute(q, t):
    """best index (the lowest on ties), best distance, second-smallest distance counting duplicates"""
    idx = np.full(len(q), -1, np.int32)
    best = np.full(len(q), regimes.NONE, np.int32)
    second = np.full(len(q), regimes.NONE, np.int32)
    if len(q) and len(t):
        d = np.zeros((len(q), len(t)), np.int32)
        for k in range(32):          # byte by byte: the whole xor cube of 128 x 4097 x 32 is not needed at once
            d += POP[q[:, None, k] ^ t[None, :, k]]
        idx[:] = d.argmin(1)
        best[:] = d.min(1)
        if len(t) > 1:
            second[:] = np.partition(d, 1, axis=1)[:, 1]
    return idx, best, second


def _near_ones(rng):
    row = np.full(32, 255, np.uint8)
    for b in rng.choice(256, 3, replace=False):
        row[b // 8] ^= np.uint8(1 << (b % 8))
    return row


@functools.lru_cache(maxsize=None)
def _pairs(npairs, t_rows, seed):
    """`npairs` pairs with `t_rows` train rows of room each: buffers of 0xFF with the live rows filled in, counts, expectation"""
    rng = np.random.default_rng(seed)
    nq = rng.integers(1, STRIDE + 1, npairs).astype(np.int32)
    nt = rng.integers(0, min(t_rows - T_SLACK, 65) + 1, npairs).astype(np.int32)
    combos = [(a, b) for b in NTS for a in NQS]
    assert len(combos) < npairs
    for p, (a, b) in enumerate(combos):
        nq[p], nt[p] = a, b
    q = np.full((npairs, Q_ROWS, 32), 255, np.uint8)
    t = np.full((npairs, t_rows, 32), 255, np.uint8)
    exp = [np.full((npairs, STRIDE), regimes.PREFILL, np.int32) for _ in range(3)]
    return rng, nq, nt, q, t, exp


def _fill(rng, q, t, exp, nq, nt, p):
    q[p, :nq[p]] = rng.integers(0, 256, (nq[p], 32), dtype=np.uint8)
    t[p, :nt[p]] = rng.integers(0, 256, (nt[p], 32), dtype=np.uint8)
    q[p, 0] = _near_ones(rng)
    q[p, nq[p] - 1] = _near_ones(rng)
    for e, o in zip(exp, brute(q[p, :nq[p]], t[p, :nt[p]])):
        e[p, :nq[p]] = o


@functools.lru_cache(maxsize=None)
def match_case(name):
    npairs, _ = MATCH_CASES[name]
    if name == "qt2_few":
        big = {24: 4096, 25: 4097}                       # behind the 24 combinations
        t_rows = 4097 + T_SLACK
        rng, nq, nt, q, t, exp = _pairs(npairs, t_rows, 7)
        for p, n in big.items():
            nt[p], nq[p] = n, (STRIDE if n == 4096 else 33)
        for p in range(npairs):
            _fill(rng, q, t, exp, nq, nt, p)
        tbuf = t.reshape(-1, 32)
    else:
        # 2047 pairs of at most 65 train rows, shared by the two cases, and a last pair whose rows run on behind the buffer's
        # regular part: it alone may be longer than the stride
        rng, nq, nt, q, t, exp = _qt4_small()
        n = int(name.split("_")[1])
        rng = np.random.default_rng(n)
        nq, nt, exp = nq.copy(), nt.copy(), [e.copy() for e in exp]
        p = npairs - 1
        nq[p], nt[p] = (STRIDE if n == 4096 else 33), n
        t_rows = t.shape[1]
        tbuf = np.full(((npairs - 1) * t_rows + n + T_SLACK, 32), 255, np.uint8)
        tbuf[:(npairs - 1) * t_rows] = t[:npairs - 1].reshape(-1, 32)
        q = q.copy()
        last_t = tbuf[p * t_rows:].reshape(1, -1, 32)
        qq = q[p:p + 1]
        _fill(rng, qq, last_t, [e[p:p + 1] for e in exp], nq[p:p + 1], nt[p:p + 1], 0)
    for a in (q, tbuf, nq, nt, *exp):
        a.setflags(write=False)
    return dict(npairs=npairs, q=q.reshape(-1, 32), t=tbuf, nq=nq, nt=nt, exp=exp, t_rows=t_rows)


@functools.lru_cache(maxsize=None)
def _qt4_small():
    npairs = 2048
    rng, nq, nt, q, t, exp = _pairs(npairs, 65 + T_SLACK, 11)
    for p in range(npairs - 1):
        _fill(rng, q, t, exp, nq, nt, p)
    return rng, nq, nt, q, t, exp


def test_match_cases_hold_their_counts_and_a_leak_would_show():
    """CPU part: every count combination is in every launch, counts differ, the regimes follow the launcher's rule as
    tests/test_match_regimes_gpu.py states it, and a 0xFF row past the counts would beat the true best match of the planted queries"""
    for name, (npairs, plan) in MATCH_CASES.items():
        c = match_case(name)
        waves4 = -(-STRIDE // 128) * npairs
        rule = (4, 1) if waves4 >= 2048 else (2, min(16, max(1, 4096 // (-(-STRIDE // 64) * npairs))))
        assert plan == rule
        have = set(zip(c["nq"].tolist(), c["nt"].tolist()))
        assert {(a, b) for a in NQS for b in NTS} <= have and len(set(c["nt"].tolist())) > len(NTS) and len(set(c["nq"].tolist())) > len(NQS)
        assert sorted(n for n in c["nt"] if n > 65) == ([4096, 4097] if name == "qt2_few" else [int(name.split("_")[1])])
        q = c["q"].reshape(npairs, Q_ROWS, 32)
        for p in range(npairs):
            n_q, n_t = int(c["nq"][p]), int(c["nt"][p])
            assert (q[p, n_q:] == 255).all()
            tp = c["t"][p * c["t_rows"]:]
            assert (tp[n_t:n_t + T_SLACK] == 255).all()          # the slack behind the live rows, and the clamped row's successor
            leak = int(POP[q[p, 0] ^ np.uint8(255)].sum())       # distance of query 0 to a garbage row: 3
            assert leak == 3 and (n_t == 0 or c["exp"][1][p, 0] > leak + 20)
            assert (c["exp"][0][p, n_q:] == regimes.PREFILL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MATCH_CASES))
@pytest.mark.parametrize("kernel", ["mfma_fp4", "mfma_i8"])
def test_match_tile_hand_over_with_garbage_tails(kernel, name, monkeypatch):
    import torch
    if regimes.ENV[kernel]:
        monkeypatch.setenv("ORBX_MATCH_KERNEL", regimes.ENV[kernel])
    else:
        monkeypatch.delenv("ORBX_MATCH_KERNEL", raising=False)
    c = match_case(name)
    npairs, want = MATCH_CASES[name]
    ex = ORBextractor(300)
    plan = regimes.match_plan(ex.handle, npairs, STRIDE)
    assert plan == want, f"{kernel} {name}: {npairs} pairs x out_stride {STRIDE} launch as (qt, nsplit) = {plan}, the case is meant for {want}"
    dev = torch.device("cuda", 0)
    dq, dt = torch.from_numpy(c["q"].copy()).to(dev), torch.from_numpy(c["t"].copy()).to(dev)
    dnq, dnt = torch.from_numpy(c["nq"].copy()).to(dev), torch.from_numpy(c["nt"].copy()).to(dev)
    out = [torch.full((npairs, STRIDE), regimes.PREFILL, dtype=torch.int32, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    _capi.check(_capi.lib().orbx_match_bruteforce_device(ex.handle, npairs, _capi.ptr(dq), _capi.ptr(dnq), Q_ROWS * 32, _capi.ptr(dt), _capi.ptr(dnt),
                                                         c["t_rows"] * 32, _capi.ptr(out[0]), _capi.ptr(out[1]), _capi.ptr(out[2]), STRIDE))
    ex.synchronize()
    got = [o.cpu().numpy() for o in out]
    ex.close()
    for g, e, what in zip(got, c["exp"], ("best index", "best distance", "second distance")):
        if not np.array_equal(g, e):
            p, qi = np.argwhere(g != e)[0]
            raise AssertionError(f"{kernel} {name} plan {plan}: {what} of pair {p} (nq {c['nq'][p]}, nt {c['nt'][p]}) query {qi}: "
                                 f"{g[p, qi]}, brute force {e[p, qi]}; {int((g != e).sum())} entries differ")
