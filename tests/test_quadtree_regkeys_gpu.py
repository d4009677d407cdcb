"""k_quadtree with register-resident keys (run with -m gpu on an MI355X): a workgroup of T threads whose level has at most
reg_keys * T candidates keeps its keys in registers, any other takes the LDS key slots or the global key map.  Whichever path a
level takes, the quadtree must return the oracle's nodes in the oracle's list order with the oracle's key each: compared per
level (debug_level_keypoints x / y in list order) and on the final keypoints and descriptors, bit for bit.

ORBX_QT_REG_KEYS (read once per handle, when it is configured) moves the register / fallback boundary; the batch size picks the
kernel instantiation by the launcher's own rule on the 256 CUs of an MI355X: 1 frame -> k_quadtree<1024>, 64 -> <512>, 130 -> <256>."""
import numpy as np
import pytest
import oracle
from orb_slam2_detailed_comments_amd import ORBextractor, synth

pytestmark = pytest.mark.gpu

QT_KPT = 6                                   # keys per thread of the register path (ORBX_QT_KPT, csrc/orbx_device.h)
THREADS_OF_BATCH = {1: 1024, 64: 512, 130: 256}
W, H, NF, NL = 640, 480, 1000, 8


class Expected:
    """what the oracle returns for one image, computed once: final result, per-level candidate counts and quadtree output"""

    def __init__(self, img, nf, cap):
        orc = oracle.OracleExtractor(nf)
        self.out = orc.extract(img, cap=cap)
        self.ncand = [len(orc.level_candidates(l)) for l in range(NL)]
        self.lkeys = [orc.level_keypoints(l) for l in range(NL)]


def check_frame(ex, res, f, exp, what):
    for l in range(NL):
        gk, ok = ex.debug_level_keypoints(l, f), exp.lkeys[l]
        assert len(gk) == len(ok), f"{what}: quadtree count level {l}: oracle {len(ok)} gpu {len(gk)}"
        assert np.array_equal(gk["x"], ok["x"]) and np.array_equal(gk["y"], ok["y"]), f"{what}: quadtree order level {l}"
    n, k, d = exp.out
    gk, gd = res
    assert n == len(gk), f"{what}: count oracle {n} gpu {len(gk)}"
    assert gk.tobytes() == k.tobytes(), f"{what}: keypoint bytes differ"
    assert np.array_equal(gd, d), f"{what}: descriptors differ"


def run(monkeypatch, img, nf, batch, knob, exp=None, **kw):
    """one handle created under ORBX_QT_REG_KEYS = knob (None: unset), `batch` copies of img in one call; frame 0 and the last
    frame against the oracle stage by stage, every other copy against frame 0.  Returns the GPU's candidate count per level."""
    if knob is None:
        monkeypatch.delenv("ORBX_QT_REG_KEYS", raising=False)
    else:
        monkeypatch.setenv("ORBX_QT_REG_KEYS", str(knob))
    h, w = img.shape
    ex = ORBextractor(nf, max_batch=batch, **kw)
    if exp is None:
        exp = Expected(img, nf, ex.max_keypoints(w, h))
    res = ex.extract_batch(np.repeat(img[None], batch, axis=0))
    what = f"{w}x{h} nf={nf} batch={batch} reg_keys={knob}"
    for f in sorted({0, batch - 1}):
        check_frame(ex, res[f], f, exp, f"{what} frame {f}")
    for f in range(1, batch - 1):
        assert res[f][0].tobytes() == res[0][0].tobytes() and np.array_equal(res[f][1], res[0][1]), f"{what}: copy {f} differs from copy 0"
    ncand = [len(ex.debug_candidates(l, 0)) for l in range(NL)]
    assert ncand == exp.ncand, f"{what}: candidate counts {ncand}, oracle {exp.ncand}"
    ex.close()
    return ncand, exp


@pytest.fixture(scope="module")
def frame():
    return synth.stream(W, H, 1, stream_id=0)[0]


@pytest.fixture(scope="module")
def frame_expected(frame):
    return Expected(frame, NF, ORBextractor(NF).max_keypoints(W, H))


@pytest.mark.parametrize("batch", sorted(THREADS_OF_BATCH))
def test_default_frame_every_knob_value_on_one_instantiation(batch, frame, frame_expected, monkeypatch):
    """case 1: the 640x480 / 1000-feature frame under ORBX_QT_REG_KEYS unset, 0, 1 and 2 on each of the three instantiations;
    on each of them some level must have taken the register path and some level the fallback"""
    T = THREADS_OF_BATCH[batch]
    took_reg = took_fallback = False
    for knob in (None, 0, 1, 2):
        ncand, _ = run(monkeypatch, frame, NF, batch, knob, frame_expected)
        reg = QT_KPT if knob is None else knob
        took_reg |= any(k <= reg * T for k in ncand) and reg > 0
        took_fallback |= any(k > reg * T for k in ncand)
    assert took_reg and took_fallback, f"k_quadtree<{T}>: register path taken {took_reg}, fallback taken {took_fallback}"


@pytest.mark.parametrize("batch", [1, 130])
def test_few_features_careful_phase_from_the_first_pass(batch, frame, monkeypatch):
    """case 2: nfeatures 20 -- a level keeps a handful of nodes, so the pass that splits the root already overshoots and the
    careful phase (largest node first, cut at N) starts at once"""
    exp = None
    for knob in (None, 0, 1):
        _, exp = run(monkeypatch, frame, 20, batch, knob, exp)


def test_no_key_and_one_key(monkeypatch):
    """case 3: a flat image (K = 0 on every level) and a single bright pixel (exactly one candidate on level 0)"""
    flat = synth.degenerate("flat", 320, 240)
    dot = np.full((240, 320), 40, np.uint8)
    dot[117, 163] = 255
    for knob in (None, 0):
        ncand, _ = run(monkeypatch, flat, 500, 1, knob)
        assert ncand == [0] * NL
        ncand, exp = run(monkeypatch, dot, 500, 1, knob)
        assert ncand[0] == 1 and exp.out[0] >= 1


def test_dense_noise_overflows_registers_to_the_global_key_map(monkeypatch):
    """case 4: uniform noise, nfeatures 4000, 256 candidates per cell: level 0 has more keys than the registers of a 1024-thread
    workgroup (6144) and than any LDS plan (4096 slots), so it takes the global key map with the register path switched on"""
    img = np.random.default_rng(42).integers(0, 256, (H, W)).astype(np.uint8)
    ncand, _ = run(monkeypatch, img, 4000, 1, None, max_cand_per_cell=256)
    assert ncand[0] > QT_KPT * 1024 and min(ncand) <= QT_KPT * 1024


# case 5: synthetic frames (stream_id, crop width of the 640x480 frame) on which one level has exactly n * T or n * T + 1
# candidates, found with the oracle; (level, count, [(reg_keys n, batch that picks T)]).  At count = n * T the level is the
# largest the registers hold, at n * T + 1 the smallest that falls back.
BOUNDARY = [
    (203, 528, 6, 512, [(2, 130), (1, 64)]),
    (200, 536, 7, 513, [(2, 130), (1, 64)]),
    (201, 416, 7, 257, [(1, 130)]),
    (200, 496, 4, 1024, [(2, 64), (1, 1)]),
    (201, 560, 2, 1025, [(2, 64), (1, 1)]),
]


@pytest.mark.parametrize("sid,cw,level,count,plans", BOUNDARY)
def test_levels_exactly_at_the_register_boundary(sid, cw, level, count, plans, monkeypatch):
    img = np.ascontiguousarray(synth.stream(W, H, 1, stream_id=sid)[0][:, :cw])
    exp = Expected(img, NF, ORBextractor(NF).max_keypoints(cw, H))
    assert exp.ncand[level] == count, f"synth drifted: level {level} of stream {sid} cropped to {cw} has {exp.ncand[level]} candidates, not {count}"
    for n, batch in plans:
        assert count - n * THREADS_OF_BATCH[batch] in (0, 1)
        run(monkeypatch, img, NF, batch, n, exp)
