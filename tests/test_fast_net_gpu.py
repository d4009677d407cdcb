"""k_fast_rows' corner test and score network (csrc/orbx_fast_net.h, both instances of fr_round) on the GPU, bit for bit against the
oracle: 16 planted frames of 160x120 through the three FAST code paths (k_fast_rows from the slab, k_fast_rows_ip in place with the
serial sequence, k_fast_rows_l0 + k_fast_rows of the FAST-first plan), three threshold pairs, and the work list at its default
length and at 64 entries (partial rounds that mix list and stack entries, the flush paths).  Per-frame counts and every keypoint's
x, y, response and octave must be equal.  A numpy model of the scheme on the level-0 image (as tests/test_fast_onepass_model.py)
shows that the planted cases are there: corners of both polarities with margin exactly th + 1, candidates at exactly th, and a
cell pair whose re-run stack passes 64 entries while list entries remain, so it is drained in the middle of a group.

Two groups per wave (k_fast_rows' gpw = 2: the second group's tile is prefetched while the first is processed, and it reuses the
first's LDS tile, score map, work list, re-run stack and corner list).  The launcher takes it from the size of the launch alone
(B x groups >= 16384, csrc/orbx_launch.h), so every comparison above also runs with ORBX_FAST_GPW=2, which pairs the groups of the
16 planted frames, and once unforced on the planted frames repeated to the smallest batch the size rule pairs.  The launcher's
group order (csrc/orbx_geometry.cpp, restated by fast_groups below): levels ascending; within a level the cell rows top to
bottom, within a row the cells left to right, a cell and its right-hand neighbour forming ONE group when their interiors
together are at most 64 + 2 columns; wave k of a launch runs groups 2k and 2k + 1 of the launch's group range."""
import ctypes as C
import numpy as np
import pytest
import oracle
import upstream_model
from orb_slam2_detailed_comments_amd import ORBextractor, synth, _capi

W, H, NF, NFEAT = 160, 120, 16, 300
W_ODD, H_ODD = 128, 96       # 9 level-0 groups of 27: every FAST launch has an odd group count (160x120: 16 of 42, all even)
PAIRS = [(20, 7), (7, 7), (100, 1)]
KNOBS = ("ORBX_PLAN", "ORBX_PLAN_SUB", "ORBX_PLAN_HEAD", "ORBX_PLAN_MIN_FRAMES", "ORBX_PIPELINE", "ORBX_PIPELINE_HEAD", "ORBX_FAST_ROOM",
         "ORBX_FORK_LEVEL", "ORBX_LEVEL0_INPLACE", "ORBX_FAST_LCAP", "ORBX_FAST_GPW")
PATHS = {"slab": {"ORBX_PLAN": "serial", "ORBX_LEVEL0_INPLACE": "0"},                    # k_fast_rows
         "inplace": {"ORBX_PLAN": "serial"},                                              # k_fast_rows_ip
         "fastfirst": {"ORBX_PLAN": "fastfirst", "ORBX_PLAN_MIN_FRAMES": "8"}}            # k_fast_rows_l0 + k_fast_rows
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
        (-2, 2), (-1, 3)]   # (dx, dy), ring index k as in fr_round's ro[] table
DOT_CONTRASTS = [(1, 2), (7, 8), (20, 21), (100, 101)]   # (th, th + 1) for every threshold of PAIRS


def _dots(bg, sign, c_left, c_right, w=W, h=H):
    """isolated single pixels on a flat ground, 10 apart (no ring holds another dot): all 16 ring pixels differ from the centre by
    the contrast, so the margin IS the contrast; the left half at c_left (= th: not a corner), the right half at c_right (th + 1)"""
    img = np.full((h, w), bg, np.int32)
    for y in range(5, h - 4, 10):
        for x in range(5, w - 4, 10):
            img[y, x] = bg + sign * (c_left if x < w // 2 else c_right)
    return img


def planted_frames(w=W, h=H):
    """(the 16 frames of the default size are the same whatever else is generated: the generator is seeded per call)"""
    W, H = w, h
    rng = np.random.default_rng(2024)
    fr = []
    for lo, hi in DOT_CONTRASTS:
        fr.append(_dots(60, +1, lo, hi, W, H))       # bright dots on dark: the ring is darker than the centre
        fr.append(_dots(200, -1, lo, hi, W, H))      # dark dots on bright
    fr.append(np.kron(rng.integers(0, 2, (-(-H // 5), -(-W // 5))), np.ones((5, 5), np.int64))[:H, :W] * 255)   # 0 / 255 blocks
    fr.append(rng.integers(0, 2, (H, W)) * 255)                                                 # 0 / 255 per pixel
    yy, xx = np.mgrid[0:H, 0:W]
    ph = (xx + yy) % 12
    st = np.where(ph == 0, 128, np.where(ph < 6, 0, 255))     # diagonal stripes, a mid-grey line between them: both pre-tests pass
    fr.append(st)
    st2 = st.copy()
    ph2 = (xx - yy) % 15
    st2[H // 2:] = np.where(ph2[H // 2:] == 0, 128, st2[H // 2:])   # lines the other way in the lower half: crossings are corners
    fr.append(st2 + rng.integers(-20, 21, (H, W)))
    fr.append(rng.integers(0, 256, (H, W)))                   # dense noise
    fr.append(rng.integers(0, 256, (H, W)) // 48 * 48)        # plateaus
    fr.extend(list(synth.stream(W, H, 2, stream_id=5).astype(np.int64)))
    assert len(fr) == NF
    return np.stack([np.clip(f, 0, 255) for f in fr]).astype(np.uint8)


def margins(img):
    """(brighter margin, darker margin, brighter compass margin mb, darker compass margin md) of every pixel 3 or more from the
    border of a level-0 image, by the definition: the maximum over the 16 arcs of the minimum over 9 of +-(ring - v)"""
    h, w = img.shape
    im = img.astype(np.int32)
    v = im[3:h - 3, 3:w - 3]
    d = [im[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - v for dx, dy in RING]
    arc = lambda s: np.max([np.min([s * d[(k + j) & 15] for j in range(9)], axis=0) for k in range(16)], axis=0)
    mb = np.minimum(np.maximum(d[0], d[8]), np.maximum(d[4], d[12]))
    md = -np.maximum(np.minimum(d[0], d[8]), np.minimum(d[4], d[12]))
    return arc(1), arc(-1), mb, md


def drains_mid_group(pre, redo, lcap=640):
    """the walk of one cell pair (rows x 64 columns of masks) with the kernel's flush rule and rounds: True when the re-run stack
    passes 64 entries while entries of the work list remain"""
    rows = pre.shape[0]
    y = 0
    while y < rows:
        n, y0 = 0, y
        while y + 7 <= rows and n + 7 * 64 <= lcap:
            n += int(pre[y:y + 7].sum()); y += 7
        while y < rows and n + 64 <= lcap:
            n += int(pre[y].sum()); y += 1
        r = redo[y0:y][pre[y0:y]]            # the list in walk order: row by row, lanes in column order
        nredo = 0
        for e0 in range(0, len(r) - 63, 64):  # full rounds
            if nredo > 64:
                return True
            nredo += int(r[e0:e0 + 64].sum())
        if nredo > 64 and len(r) % 64:         # the rest of the list waits for a round of stack entries alone
            return True
    return False


def fast_groups(w, h, nfeat=NFEAT):
    """the launcher's FAST groups of a w x h frame, in launch order (orbx_build_geometry, csrc/orbx_geometry.cpp): a list of
    (level, [cells]) with cells (x0, y0, cw, ch) in the padded level's coordinates; the interior of a cell (where corners are
    reported) is [x0 + 3, x0 + cw - 3) x [y0 + 3, y0 + ch - 3)"""
    out = []
    for l, g in enumerate(upstream_model.geometry(w, h, nfeat, padded=True)):
        cells = [c[:4] for c in g["cells"] if c[2] >= 7 and c[3] >= 7]     # in push order: rows top to bottom, columns left to right
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


def group_counts(w, h):
    g = fast_groups(w, h)
    return sum(1 for l, _ in g if l == 0), len(g)


def split_batch(b, s, head=False):
    """orbx_split_batch of csrc/orbx_internal.h: the frames of each sub-batch"""
    units = 2 * s - 1 if head else s
    off = [0]
    while len(off) < s:
        share = (b * (2 if head and len(off) > 1 else 1) // units) & ~7
        nxt = off[-1] + max(share, 8)
        if b - nxt < 8:
            break
        off.append(nxt)
    off.append(b)
    return [off[k + 1] - off[k] for k in range(len(off) - 1)]


def fast_launches(path, nframes, w, h):
    """(frames, groups) of every k_fast_rows launch of one batch call on `path`"""
    l0, total = group_counts(w, h)
    if path != "fastfirst":
        return [(nframes, total)]
    return [(nframes, l0)] + [(b, total - l0) for b in split_batch(nframes, 3)]     # plan_sub = 3 (csrc/orbx_handle.h)


def fast_gpw(ex, nframes, ngroups):
    gpw = C.c_int(-1)
    _capi.check(_capi.lib().orbx_debug_fast_gpw(ex.handle, nframes, ngroups, C.byref(gpw)))
    return gpw.value


def level0_corner_counts(img, th):
    """corners (margin of either polarity > th) of every cell of every level-0 group of one frame, on the padded level 0 (the
    frame with its 19-pixel reflect-101 border): [[count per cell] per group]"""
    a = margins(np.pad(img, 19, mode="reflect"))            # index [y - 3, x - 3] of the padded image
    m = np.maximum(a[0], a[1])
    return [[int((m[y0:y0 + ch - 6, x0:x0 + cw - 6] > th).sum()) for x0, y0, cw, ch in cells] for l, cells in fast_groups(W, H) if l == 0]


@pytest.fixture(scope="module")
def planted():
    frames = planted_frames()
    ref = {}
    for ini, mn in PAIRS:
        orc = oracle.OracleExtractor(NFEAT, 1.2, 8, ini, mn)
        ref[ini, mn] = [orc.extract(frames[f])[:2] for f in range(NF)]
    return frames, ref


def test_planted_cases_exist():
    """CPU part: the frames hold what the GPU comparison is meant to see (a test that plants nothing passes for nothing)"""
    frames = planted_frames()
    m = [margins(f) for f in frames]
    for th in sorted({t for p in PAIRS for t in p}):
        for pol in (0, 1):
            assert any((a[pol] == th + 1).any() for a in m), f"no corner of polarity {pol} with margin exactly {th + 1}"
        # a candidate (it passes the walk's pre-test) whose larger margin is exactly th: not a corner
        assert any(((np.maximum(a[2], a[3]) > th) & (np.maximum(a[0], a[1]) == th)).any() for a in m), f"no candidate at exactly {th}"
    # level 0 of 160x120: cells of 32 x 44 interior pixels from pixel (19, 19), two pairs of 64 columns, two cell rows
    drained = False
    for ini in sorted({p[0] for p in PAIRS}):
        for a in m:
            mar = np.where(a[3] > a[2], a[1], a[0])                 # margin of the polarity taken first
            pre = np.maximum(a[2], a[3]) > ini
            redo = pre & (np.minimum(a[2], a[3]) > ini) & ~(mar > ini)
            for y0 in (16, 60):                                      # the margin arrays start at pixel (3, 3)
                for x0 in (16, 80):
                    drained |= drains_mid_group(pre[y0:y0 + 44, x0:x0 + 64], redo[y0:y0 + 44, x0:x0 + 64])
    assert drained, "no cell pair with 65 or more re-run candidates ahead of remaining list entries"
    # ---- two groups per wave: what the first group of a wave leaves behind must differ from what the second needs.  Level 0 of
    # the padded 198 x 158 frame: four rows of five cells (34-column interiors, the last 24), four groups per row -- three single
    # cells and the pair of the last two -- so a row is two waves and a wave never spans two rows.  Level 0 comes first in every
    # launch that has it, so wave k holds level-0 groups 2k and 2k + 1 on all three paths.
    l0, total = group_counts(W, H)
    assert (l0, total) == (16, 42) and [len(c) for lv, c in fast_groups(W, H)[:4]] == [1, 1, 1, 2]
    # (the walk above cuts the un-padded frame into 64-column pieces; on the launcher's groups the stack is drained mid-group as
    # well, in a wave's first group and in a wave's second)
    drained = set()
    for ini in sorted({p[0] for p in PAIRS}):
        for f in frames:
            a = margins(np.pad(f, 19, mode="reflect"))
            mar = np.where(a[3] > a[2], a[1], a[0])
            pre = np.maximum(a[2], a[3]) > ini
            redo = pre & (np.minimum(a[2], a[3]) > ini) & ~(mar > ini)
            for k, (lv, cells) in enumerate(fast_groups(W, H)[:l0]):
                x0, y0, ch = cells[0][0], cells[0][1], cells[0][3]
                n = min(cells[-1][0] + cells[-1][2] - 6 - x0, 64)
                if drains_mid_group(pre[y0:y0 + ch - 6, x0:x0 + n], redo[y0:y0 + ch - 6, x0:x0 + n]):
                    drained.add(k % 2)
    assert drained == {0, 1}, "the re-run stack is not drained mid-group in both positions of a wave"
    ccap = 64                                                # the corner list of a group at ORBX_FAST_LCAP=64 (min(lcap, 512))
    found = dict(a=set(), b=set(), c=set())
    for ini, mn in PAIRS:
        for f in frames:
            cc = level0_corner_counts(f, ini)
            for k in range(0, l0, 2):
                n0, n1 = sum(cc[k]), sum(cc[k + 1])
                if n0 > ccap >= n1:
                    found["a"].add(ini)                      # the first group takes the dense rescan, the second the corner list
                if n1 > ccap >= n0:
                    found["b"].add(ini)
                if ini != mn and (min(cc[k]) == 0) != (min(cc[k + 1]) == 0):
                    found["c"].add(ini)                      # exactly one of the two has a cell without a corner: its minThFAST re-run
    assert found["a"], "no wave whose first group alone exceeds the corner list at ORBX_FAST_LCAP=64"
    assert found["b"] == {p[0] for p in PAIRS}, "no wave whose second group alone exceeds the corner list, at some iniThFAST"
    assert found["c"] == {p[0] for p in PAIRS if p[0] != p[1]}, "no wave in which exactly one group re-runs a cell at minThFAST"
    # (d) a last wave with one group: the group counts are the geometry's, not the frames', and 160x120 has 16 / 26 / 42 groups in
    # its launches, all even -- no planted frame can change that.  The same 16 frames generated at 128x96 have 9 / 18 / 27
    # (test_odd_group_count_with_forced_pairs below).
    assert all(n % 2 == 0 for b, n in fast_launches("slab", NF, W, H) + fast_launches("fastfirst", NF, W, H))
    assert group_counts(W_ODD, H_ODD) == (9, 27)
    assert [n % 2 for b, n in fast_launches("inplace", NF, W_ODD, H_ODD) + fast_launches("fastfirst", NF, W_ODD, H_ODD)] == [1, 1, 0, 0]
    assert fast_launches("fastfirst", NF, W, H) == [(16, 16), (8, 26), (8, 26)]


def _run_path(monkeypatch, path, pair, lcap, gpw, frames, w=W, h=H, repeat=1):
    """fresh handle under the path's knobs, one device call over `frames` repeated `repeat` times on the device; asserts the
    groups per wave of every FAST launch of the call (the forced value, else the size rule) and returns the device outputs
    (keypoints, descriptors, counts) and the gpw the launches took"""
    import torch
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    if lcap:
        monkeypatch.setenv("ORBX_FAST_LCAP", lcap)
    if gpw:
        monkeypatch.setenv("ORBX_FAST_GPW", gpw)
    n = len(frames) * repeat
    ex = ORBextractor(NFEAT, 1.2, 8, pair[0], pair[1], max_batch=n)
    ex.profile_enable(1 << _capi.K_NAMES.index("k_fast_rows"))     # one bit: counts the FAST launches, leaves the plan as it is
    cap = ex.max_keypoints(w, h)
    dev = torch.device("cuda", 0)
    imgs = torch.from_numpy(frames).to(dev).repeat(repeat, 1, 1)
    kps = torch.zeros((n, cap * 28), dtype=torch.uint8, device=dev)
    desc = torch.zeros((n, cap * 32), dtype=torch.uint8, device=dev)
    cnt = torch.full((n,), -3, dtype=torch.int32, device=dev)
    st = torch.full((n,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ex.extract_batch_device(imgs, n, w, h, imgs.stride(1), imgs.stride(0), kps, desc, cnt, st, cap)
    ex.synchronize()
    launches = ex.profile_read()["k_fast_rows"][1]
    l0, total = C.c_int(0), C.c_int(0)
    _capi.check(_capi.lib().orbx_debug_fast_groups(ex.handle, C.byref(l0), C.byref(total)))
    assert (l0.value, total.value) == group_counts(w, h), "the group model of this file is not the library's geometry"
    plan = fast_launches(path, n, w, h)
    took = [fast_gpw(ex, b, ng) for b, ng in plan]
    assert not st.cpu().numpy().any()
    ex.close()
    assert launches == len(plan), f"{path}: {launches} FAST launches, modelled {plan}"
    want = int(gpw) if gpw else None
    for (b, ng), g in zip(plan, took):
        rule = 2 if b * ng >= 16384 else 1
        assert g == (want or rule), f"{path} ORBX_FAST_GPW={gpw}: the launch of {b} frames x {ng} groups runs {g} groups per wave"
    return kps, desc, cnt, took


def _assert_oracle(got_n, got_k, ref, what):
    total = 0
    for f in range(len(ref)):
        n, k = ref[f]
        assert got_n[f] == n, f"{what} frame {f}: count {got_n[f]} oracle {n}"
        for field in ("x", "y", "response", "octave"):
            assert got_k[f, :n][field].tobytes() == k[field].tobytes(), f"{what} frame {f}: {field} differs"
        total += n
    assert total > 0


@pytest.mark.gpu
@pytest.mark.parametrize("lcap,gpw", [(None, None), ("64", None), (None, "2"), ("64", "2")], ids=["None", "64", "None-gpw2", "64-gpw2"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"th{p[0]}_{p[1]}")
@pytest.mark.parametrize("path", list(PATHS))
def test_fast_paths_equal_the_oracle(path, pair, lcap, gpw, planted, monkeypatch):
    """gpw None: one group per wave (16 frames are far below the size rule); "2": ORBX_FAST_GPW=2 pairs the planted groups"""
    frames, ref = planted
    kps, _, cnt, took = _run_path(monkeypatch, path, pair, lcap, gpw, frames)
    assert set(took) == ({2} if gpw else {1}) and (len(took) > 1) == (path == "fastfirst")
    _assert_oracle(cnt.cpu().numpy(), kps.cpu().numpy().view(_capi.KP_DTYPE), ref[pair], f"{path} {pair} lcap {lcap} gpw {took}")


@pytest.fixture(scope="module")
def planted_odd():
    frames = planted_frames(W_ODD, H_ODD)
    orc = oracle.OracleExtractor(NFEAT, 1.2, 8, 20, 7)
    return frames, [orc.extract(frames[f])[:2] for f in range(NF)]


@pytest.mark.gpu
@pytest.mark.parametrize("lcap", [None, "64"])
@pytest.mark.parametrize("path", list(PATHS))
def test_odd_group_count_with_forced_pairs(path, lcap, planted_odd, monkeypatch):
    """the planted frames at 128x96, ORBX_FAST_GPW=2: 27 groups in the serial launches, 9 in the level-0 launch of the FAST-first
    plan -- the last wave of those launches has ONE group and must not run on into the next group of the table"""
    frames, ref = planted_odd
    kps, _, cnt, took = _run_path(monkeypatch, path, (20, 7), lcap, "2", frames, W_ODD, H_ODD)
    assert set(took) == {2} and fast_launches(path, NF, W_ODD, H_ODD)[0][1] % 2 == 1
    _assert_oracle(cnt.cpu().numpy(), kps.cpu().numpy().view(_capi.KP_DTYPE), ref, f"128x96 {path} lcap {lcap} gpw {took}")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["slab", "inplace"])
def test_size_rule_pairs_the_planted_groups(path, planted, monkeypatch):
    """ORBX_FAST_GPW unset, ORBX_PLAN=serial, both level-0 modes: the 16 planted frames repeated on the device to the smallest
    multiple of 16 at which the launcher itself takes two groups per wave (frames x 42 groups >= 16384: 400 frames, one launch).
    The first 16 frames equal the oracle and every copy is byte-identical to its first occurrence."""
    frames, ref = planted
    pair = PAIRS[0]
    total = group_counts(W, H)[1]
    rep = -(-16384 // (total * NF))
    assert rep * NF == 400 and (rep - 1) * NF * total < 16384 <= rep * NF * total
    kps, desc, cnt, took = _run_path(monkeypatch, path, pair, None, None, frames, repeat=rep)
    assert took == [2], f"{path}: {rep * NF} frames x {total} groups run {took} groups per wave without the knob"
    for t in (kps, desc, cnt.view(-1, 1)):
        v = t.view(rep, NF, -1)
        assert bool((v == v[0:1]).all()), "a repeated frame came out differently from its first occurrence"
    _assert_oracle(cnt[:NF].cpu().numpy(), kps[:NF].cpu().numpy().view(_capi.KP_DTYPE), ref[pair], f"{path} x {rep * NF} frames gpw {took}")


@pytest.mark.gpu
def test_gpw_knob_rejects_other_values(planted, monkeypatch):
    """ORBX_FAST_GPW is 1 or 2; anything else is refused when the handle is configured, before any launch"""
    from orb_slam2_detailed_comments_amd import OrbxError
    frames, _ = planted
    for bad in ("0", "3", "two"):
        with pytest.raises(OrbxError) as e:
            _run_path(monkeypatch, "inplace", PAIRS[0], None, bad, frames)
        assert e.value.status == _capi.BAD_ARGUMENT and "ORBX_FAST_GPW" in str(e.value), bad
