"""k_fast_rows' corner test and score network (csrc/orbx_fast_net.h, both instances of fr_round) on the GPU, bit for bit against the
oracle: 16 planted frames of 160x120 through the three FAST code paths (k_fast_rows from the slab, k_fast_rows_ip in place with the
serial sequence, k_fast_rows_l0 + k_fast_rows of the FAST-first plan), three threshold pairs, and the work list at its default
length and at 64 entries (partial rounds that mix list and stack entries, the flush paths).  Per-frame counts and every keypoint's
x, y, response and octave must be equal.  A numpy model of the scheme on the level-0 image (as tests/test_fast_onepass_model.py)
shows that the planted cases are there: corners of both polarities with margin exactly th + 1, candidates at exactly th, and a
cell pair whose re-run stack passes 64 entries while list entries remain, so it is drained in the middle of a group."""
import numpy as np
import pytest
import oracle
from orb_slam2_detailed_comments_amd import ORBextractor, synth, _capi

W, H, NF, NFEAT = 160, 120, 16, 300
PAIRS = [(20, 7), (7, 7), (100, 1)]
KNOBS = ("ORBX_PLAN", "ORBX_PLAN_SUB", "ORBX_PLAN_HEAD", "ORBX_PLAN_MIN_FRAMES", "ORBX_PIPELINE", "ORBX_PIPELINE_HEAD", "ORBX_FAST_ROOM",
         "ORBX_FORK_LEVEL", "ORBX_LEVEL0_INPLACE", "ORBX_FAST_LCAP")
PATHS = {"slab": {"ORBX_PLAN": "serial", "ORBX_LEVEL0_INPLACE": "0"},                    # k_fast_rows
         "inplace": {"ORBX_PLAN": "serial"},                                              # k_fast_rows_ip
         "fastfirst": {"ORBX_PLAN": "fastfirst", "ORBX_PLAN_MIN_FRAMES": "8"}}            # k_fast_rows_l0 + k_fast_rows
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
        (-2, 2), (-1, 3)]   # (dx, dy), ring index k as in fr_round's ro[] table
DOT_CONTRASTS = [(1, 2), (7, 8), (20, 21), (100, 101)]   # (th, th + 1) for every threshold of PAIRS


def _dots(bg, sign, c_left, c_right):
    """isolated single pixels on a flat ground, 10 apart (no ring holds another dot): all 16 ring pixels differ from the centre by
    the contrast, so the margin IS the contrast; the left half at c_left (= th: not a corner), the right half at c_right (th + 1)"""
    img = np.full((H, W), bg, np.int32)
    for y in range(5, H - 4, 10):
        for x in range(5, W - 4, 10):
            img[y, x] = bg + sign * (c_left if x < W // 2 else c_right)
    return img


def planted_frames():
    rng = np.random.default_rng(2024)
    fr = []
    for lo, hi in DOT_CONTRASTS:
        fr.append(_dots(60, +1, lo, hi))       # bright dots on dark: the ring is darker than the centre
        fr.append(_dots(200, -1, lo, hi))      # dark dots on bright
    fr.append(np.kron(rng.integers(0, 2, (H // 5, W // 5)), np.ones((5, 5), np.int64)) * 255)   # 0 / 255 blocks
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


@pytest.mark.gpu
@pytest.mark.parametrize("lcap", [None, "64"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"th{p[0]}_{p[1]}")
@pytest.mark.parametrize("path", list(PATHS))
def test_fast_paths_equal_the_oracle(path, pair, lcap, planted, monkeypatch):
    import torch
    frames, ref = planted
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    if lcap:
        monkeypatch.setenv("ORBX_FAST_LCAP", lcap)
    ex = ORBextractor(NFEAT, 1.2, 8, pair[0], pair[1], max_batch=NF)
    ex.profile_enable(1 << _capi.K_NAMES.index("k_fast_rows"))     # one bit: counts the FAST launches, leaves the plan as it is
    cap = ex.max_keypoints(W, H)
    dev = torch.device("cuda", 0)
    imgs = torch.from_numpy(frames).to(dev)
    kps = torch.zeros((NF, cap * 28), dtype=torch.uint8, device=dev)
    desc = torch.zeros((NF, cap * 32), dtype=torch.uint8, device=dev)
    cnt = torch.full((NF,), -3, dtype=torch.int32, device=dev)
    st = torch.full((NF,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ex.extract_batch_device(imgs, NF, W, H, imgs.stride(1), imgs.stride(0), kps, desc, cnt, st, cap)
    ex.synchronize()
    launches = ex.profile_read()["k_fast_rows"][1]
    got_n, got_k = cnt.cpu().numpy(), kps.cpu().numpy().view(_capi.KP_DTYPE)
    assert not st.cpu().numpy().any()
    ex.close()
    assert (launches > 1) == (path == "fastfirst"), f"{path}: {launches} FAST launches"
    total = 0
    for f in range(NF):
        n, k = ref[pair][f]
        assert got_n[f] == n, f"{path} {pair} lcap {lcap} frame {f}: count {got_n[f]} oracle {n}"
        for field in ("x", "y", "response", "octave"):
            assert got_k[f, :n][field].tobytes() == k[field].tobytes(), f"{path} {pair} lcap {lcap} frame {f}: {field} differs"
        total += n
    assert total > 0
