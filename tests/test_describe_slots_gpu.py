"""k_describe indexes its waves by slot of the per-frame level-keypoint table: the level of a slot comes from the
kp_begin values, a slot beyond its level's count is a dead wave, the output position is the sum of the counts below + the index.
Everything that prologue can get wrong shows in the output rows, so every case below compares keypoints, descriptors, counts and
status of every frame with the CPU oracle, at the smallest shapes where the condition occurs -- and asserts that it does occur."""
import numpy as np
import pytest
import oracle
from orb_slam2_detailed_comments_amd import ORBextractor, synth, _capi

pytestmark = pytest.mark.gpu

FP = {"fma": _capi.FP_GCC_FMA, "strict": _capi.FP_STRICT}
OFP = {"fma": oracle.FP_GCC_FMA, "strict": oracle.FP_STRICT}
EDGE_FAST = 16   # EDGE_THRESHOLD - 3: first / last column and row FAST looks at (src/ORBextractor.cc:1466-1469)


def corner_image(w, h, seed, cell, amp, smooth):
    """flat grey with value noise of `cell` pixels and amplitude `amp` in the top-left quarter, box-smoothed `smooth` times"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 128.0)
    gh, gw = (h // 2 + cell - 1) // cell, (w // 2 + cell - 1) // cell
    tex = np.kron(rng.integers(-amp, amp + 1, (gh, gw)).astype(np.float64), np.ones((cell, cell)))[:h // 2, :w // 2]
    img[:h // 2, :w // 2] += tex
    for _ in range(smooth):
        p = np.pad(img, 1, mode="edge")
        img = (p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] + 4 * p[1:-1, 1:-1]) / 8
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


_ORACLE = {}


def reference(key, frames, nf, nl, fp):
    """oracle rows of every frame, computed once per (image set, parameters) and shared: (n, keypoints, descriptors, the
    extractor's level widths)"""
    k = (key, nf, nl, fp)
    if k not in _ORACLE:
        rows = []
        for img in frames:
            orc = oracle.OracleExtractor(nf, 1.2, nl, 20, 7, OFP[fp])
            n, kp, d = orc.extract(np.ascontiguousarray(img), cap=1 << 14)
            assert n >= 0
            lw = [orc.level_image(l).shape[1] for l in range(nl)]
            rows.append((n, kp if n else np.zeros(0, _capi.KP_DTYPE), d if n else np.zeros((0, 32), np.uint8), lw))
        _ORACLE[k] = rows
    return _ORACLE[k]


def level_counts(ref_row, nl):
    return np.bincount(ref_row[1]["octave"], minlength=nl)


def run_device(monkeypatch, frames, nf, nl, fp, inplace, cap=None, stride=None):
    """one device-pointer call on a fresh handle with max_batch = the batch; returns counts, status, keypoint and descriptor rows"""
    import torch
    frames = np.ascontiguousarray(frames)
    b, h, w = frames.shape
    stride = stride or w
    monkeypatch.delenv("ORBX_LEVEL0_INPLACE", raising=False)
    if not inplace:
        monkeypatch.setenv("ORBX_LEVEL0_INPLACE", "0")
    ex = ORBextractor(nf, 1.2, nl, 20, 7, fp_mode=FP[fp], max_batch=b)
    total_cap = ex.max_keypoints(w, h)
    cap = cap or total_cap
    dev = torch.device("cuda", 0)
    host = np.full((b, h, stride), 0xEE, np.uint8)
    host[:, :, :w] = frames
    imgs = torch.from_numpy(host).to(dev)
    kps = torch.full((b, cap * 28), 0xA5, dtype=torch.uint8, device=dev)
    desc = torch.full((b, cap * 32), 0x5A, dtype=torch.uint8, device=dev)
    cnt = torch.full((b,), -3, dtype=torch.int32, device=dev)
    st = torch.full((b,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ex.extract_batch_device(imgs, b, w, h, stride, h * stride, kps, desc, cnt, st, cap)
    ex.synchronize()
    out = dict(cnt=cnt.cpu().numpy(), st=st.cpu().numpy(), kps=kps.cpu().numpy(), desc=desc.cpu().numpy(), cap=cap,
               fpl=ex.features_per_level(), total_cap=total_cap)
    ex.close()
    return out


def assert_equal_oracle(out, ref, what):
    cap = out["cap"]
    for f, (n, kp, d, _) in enumerate(ref):
        m = min(n, cap)
        assert int(out["cnt"][f]) == m, f"{what}: count of frame {f}: {int(out['cnt'][f])} != {m}"
        assert int(out["st"][f]) == (_capi.CAPACITY if n > cap else 0), f"{what}: status of frame {f} = {int(out['st'][f])}"
        assert out["kps"][f][:m * 28].tobytes() == kp[:m].tobytes(), f"{what}: keypoints of frame {f} differ from the oracle"
        assert out["desc"][f][:m * 32].tobytes() == d[:m].tobytes(), f"{what}: descriptors of frame {f} differ from the oracle"
        # rows at and beyond the count are not written
        assert (out["kps"][f][m * 28:] == 0xA5).all() and (out["desc"][f][m * 32:] == 0x5A).all(), f"{what}: frame {f} wrote beyond its count"


def kp_caps(fpl, lw, h_of_w):
    """kp_cap of every level as the library sizes its table: max(nfeat + 3, 4 * nIni), nIni = round(width / height) of the FAST
    region (src/ORBextractor.cc:1010)"""
    caps = []
    for l, w in enumerate(lw):
        rw, rh = w - 2 * EDGE_FAST, h_of_w[l] - 2 * EDGE_FAST
        nini = max(int(np.floor(rw / rh + 0.5)), 1) if rw > 0 and rh > 0 else 1
        caps.append(max(int(fpl[l]) + 3, 4 * nini))
    return caps


# (cell, amp, smooth, seed) of corner_image at 96 x 80, 200 features, found with the oracle
SPARSE = [(3, 20, 4, 2),    # levels 0-4 and 6 hold keypoints, level 5 none
          (4, 10, 0, 0),    # level 0 empty, levels 1-3 not
          (6, 10, 0, 5)]    # level 0 empty and level 5 empty below level 6


def sparse_frames():
    return np.stack([corner_image(96, 80, s, c, a, m) for c, a, m, s in SPARSE])


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "eager"])
@pytest.mark.parametrize("fp", ["fma", "strict"])
def test_empty_levels(monkeypatch, fp, inplace):
    frames = sparse_frames()
    ref = reference("sparse", frames, 200, 8, fp)
    c = [level_counts(r, 8) for r in ref]
    assert c[0][5] == 0 and c[0][4] > 0 and c[0][6] > 0, c[0]          # an empty level between two non-empty ones
    assert c[1][0] == 0 and c[1][1:].sum() > 0, c[1]                   # level 0 empty
    assert c[2][0] == 0 and c[2][5] == 0 and c[2][4] > 0 and c[2][6] > 0, c[2]
    assert_equal_oracle(run_device(monkeypatch, frames, 200, 8, fp, inplace), ref, f"sparse {fp} inplace={inplace}")


def full_frames(w, h, n, sid):
    return synth.stream(w, h, n, stream_id=sid)


def test_level_filled_to_kp_cap(monkeypatch):
    """few features asked of a textured image: the quadtree of a level returns more than its share, up to the table's kp_cap"""
    frames, nf = full_frames(96, 80, 3, 700), 12
    ref = reference("capfill", frames, nf, 8, "fma")
    out = run_device(monkeypatch, frames, nf, 8, "fma", True)
    orc = oracle.OracleExtractor(nf)
    orc.extract(frames[0])
    dims = [orc.level_image(l).shape for l in range(8)]
    caps = kp_caps(out["fpl"], [d[1] for d in dims], [d[0] for d in dims])
    assert sum(caps) == out["total_cap"], (caps, out["total_cap"])   # the restated kp_cap is the library's
    filled = [(f, l) for f, r in enumerate(ref) for l, n in enumerate(level_counts(r, 8)) if n == caps[l]]
    assert filled, [level_counts(r, 8).tolist() for r in ref]
    assert_equal_oracle(out, ref, "kp_cap")


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "eager"])
def test_total_beyond_callers_cap(monkeypatch, inplace):
    frames = np.concatenate([full_frames(96, 80, 2, 710), sparse_frames()[:1]])
    ref = reference("cap", frames, 200, 8, "fma")
    cap = ref[0][0] // 2
    assert ref[0][0] > cap and ref[1][0] > cap and 0 < ref[2][0] <= cap, [r[0] for r in ref]   # two frames clamped, one not
    assert_equal_oracle(run_device(monkeypatch, frames, 200, 8, "fma", inplace, cap=cap), ref, f"cap {cap} inplace={inplace}")


@pytest.mark.parametrize("fp", ["fma", "strict"])
@pytest.mark.parametrize("nl", [4, 5])
def test_other_level_counts(monkeypatch, nl, fp):
    """nlevels != 8: the general loop of the prologue"""
    frames = np.concatenate([full_frames(128, 96, 2, 720), corner_image(128, 96, 1, 4, 40, 0)[None]])
    ref = reference("nl", frames, 300, nl, fp)
    assert all(r[0] > 0 for r in ref) and all((level_counts(r, nl) > 0).all() for r in ref[:2])
    assert_equal_oracle(run_device(monkeypatch, frames, 300, nl, fp, True), ref, f"{nl} levels {fp}")


@pytest.mark.parametrize("B", [1, 7, 9])
def test_partial_frame_groups(monkeypatch, B):
    """frames are dealt in groups of eight: the last group of these batches is not full"""
    frames = np.concatenate([full_frames(96, 80, 6, 730), sparse_frames()])[:B]
    ref = reference("groups", np.concatenate([full_frames(96, 80, 6, 730), sparse_frames()]), 200, 8, "fma")[:B]
    assert_equal_oracle(run_device(monkeypatch, frames, 200, 8, "fma", True), ref, f"batch {B}")


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "eager"])
@pytest.mark.parametrize("fp", ["fma", "strict"])
@pytest.mark.parametrize("w", [96, 97, 98, 99])
def test_right_edge_tail(monkeypatch, w, fp, inplace):
    """w & 3 = 0..3 with keypoints within 18 px of the right edge of their level: their taps reach the last w & 3 columns' side of
    the blur (the tail path of the tap code)"""
    frames = full_frames(w, 80, 2, 740 + w)
    ref = reference(f"edge{w}", frames, 300, 8, fp)
    assert w & 3 == w - 96
    scale = 1.2 ** np.arange(8)
    near = 0
    for n, kp, _, lw in ref:
        xl = np.rint(kp["x"] / scale[kp["octave"]].astype(np.float32)).astype(int)
        near += int((xl + 18 >= (np.asarray(lw)[kp["octave"]] & ~3)).sum())
    assert near > 0, f"no keypoint within 18 px of the right edge at width {w}"
    out = run_device(monkeypatch, frames, 300, 8, fp, inplace, stride=(w + 3) & ~3)
    assert_equal_oracle(out, ref, f"width {w} {fp} inplace={inplace}")
