"""The FAST-first launch plan of the batched extraction (csrc/orbx_extract.cpp run_chunk, ORBX_PLAN=fastfirst): FAST over the level-0
groups of the whole batch starts at once on the main stream, the resize chains of the sub-batches run beside it on the side
stream, the FAST groups of levels >= 1 follow per sub-batch, quadtree and descriptors once over the batch.  The plan changes
launch order, residency and which FAST kernel runs, nothing else: against ORBX_PLAN=serial on a fresh handle every keypoint,
descriptor, count, status word and the t vs t-1 match must be equal byte for byte."""
import ctypes as C
import numpy as np
import pytest
import oracle
from orb_slam2_detailed_comments_amd import ORBextractor, synth, _capi

pytestmark = pytest.mark.gpu

KNOBS = ("ORBX_PLAN", "ORBX_PLAN_SUB", "ORBX_PLAN_HEAD", "ORBX_PLAN_MIN_FRAMES", "ORBX_PIPELINE", "ORBX_PIPELINE_HEAD",
         "ORBX_FAST_ROOM", "ORBX_FORK_LEVEL", "ORBX_LEVEL0_INPLACE")
FAST_BIT = 1 << _capi.K_NAMES.index("k_fast_rows")
SERIAL = {"ORBX_PLAN": "serial"}


def _plan(sub, **more):
    return dict({"ORBX_PLAN": "fastfirst", "ORBX_PLAN_MIN_FRAMES": "8", "ORBX_PLAN_SUB": str(sub)}, **more)


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _device(frames, stride=None):
    """frames [B,H,W] or [B,H,W,C] -> device tensor [B,H,stride] whose bytes between the row's end and `stride` are 0xEE"""
    import torch
    b, h = frames.shape[:2]
    row = frames.reshape(b, h, -1)
    stride = stride or row.shape[2]
    host = np.full((b, h, stride), 0xEE, np.uint8)
    host[:, :, :row.shape[2]] = row
    return torch.from_numpy(host).to(torch.device("cuda", 0))


def _buffers(n, cap):
    import torch
    dev = torch.device("cuda", 0)
    out = dict(kps=torch.full((n, cap * 28), 0xA5, dtype=torch.uint8, device=dev), desc=torch.full((n, cap * 32), 0x5A, dtype=torch.uint8, device=dev),
               cnt=torch.full((n,), -3, dtype=torch.int32, device=dev), st=torch.full((n,), -5, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()   # the fills ran on torch's stream, which is not ordered with the handle's
    return out


def _extract(ex, imgs, w, h, out, cap):
    ex.extract_batch_device(imgs, imgs.shape[0], w, h, imgs.stride(1), imgs.stride(0), out["kps"], out["desc"], out["cnt"], out["st"], cap)


def _match(ex, out, cap):
    """frame t against t-1 on the device, added to `out`"""
    import torch
    n = out["cnt"].shape[0]
    ex.synchronize()
    tr_desc = torch.roll(out["desc"], 1, 0).contiguous(); tr_cnt = torch.roll(out["cnt"], 1, 0).contiguous()
    mi = torch.full((n, cap), -7, dtype=torch.int32, device=tr_desc.device); mb = torch.zeros_like(mi); ms = torch.zeros_like(mi)
    torch.cuda.synchronize()
    _capi.check(_capi.lib().orbx_match_bruteforce_device(ex.handle, n, _capi.ptr(out["desc"]), _capi.ptr(out["cnt"]), cap * 32, _capi.ptr(tr_desc),
                                                         _capi.ptr(tr_cnt), cap * 32, _capi.ptr(mi), _capi.ptr(mb), _capi.ptr(ms), cap))
    out.update(mi=mi, mb=mb, ms=ms)


def _groups(ex):
    l0, total = C.c_int(0), C.c_int(0)
    _capi.check(_capi.lib().orbx_debug_fast_groups(ex.handle, C.byref(l0), C.byref(total)))
    return l0.value, total.value


def _run(monkeypatch, env, imgs, w, h, nf, fmt=None, profile=FAST_BIT):
    """fresh handle under `env`, one device-pointer call, the match; returns (outputs, FAST launches, (level-0 groups, groups)).
    The one-bit FAST profile leaves the launch plan as it is and counts the plan's FAST launches."""
    _env(monkeypatch, env)
    n = imgs.shape[0]
    ex = ORBextractor(nf, max_batch=n)
    if fmt is not None:
        ex.set_input_format(fmt)
    ex.profile_enable(profile)
    cap = ex.max_keypoints(w, h)
    out = _buffers(n, cap)
    _extract(ex, imgs, w, h, out, cap)
    _match(ex, out, cap)
    ex.synchronize()
    launches = ex.profile_read()["k_fast_rows"][1]
    groups = _groups(ex)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    ex.close()
    return res, launches, groups


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    assert (a["cnt"] > 0).all(), what
    assert not a["st"].any(), what
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs from the serial sequence"


def _sub_batches(n, sub, head=True):
    """orbx_split_batch of csrc/orbx_internal.h"""
    units = 2 * sub - 1 if head else sub
    off = [0]
    while len(off) < sub:
        share = (n * (2 if head and len(off) > 1 else 1) // units) & ~7
        nxt = off[-1] + max(share, 8)
        if n - nxt < 8:
            break
        off.append(nxt)
    return len(off)


def _oracle(out, frames, nf, what):
    cap = out["kps"].shape[1] // 28
    for f in (0, len(frames) - 1):
        n, k, d = oracle.OracleExtractor(nf).extract(np.ascontiguousarray(frames[f]), cap=cap)
        assert n == int(out["cnt"][f]), (what, f)
        assert out["kps"][f][:n * 28].tobytes() == k.tobytes(), f"{what}: keypoints of frame {f} differ from the oracle"
        assert out["desc"][f][:n * 32].tobytes() == d.tobytes(), f"{what}: descriptors of frame {f} differ from the oracle"


# (width, height, row stride, nfeatures): the in-place minimum; an odd size with row padding; a quarter-VGA frame
SMALL = [(64, 64, 64, 200), (97, 75, 100, 1000), (320, 240, 320, 500)]


@pytest.mark.parametrize("n", [13, 24])
@pytest.mark.parametrize("w,h,stride,nf", SMALL)
def test_small_geometries_equal_serial(w, h, stride, nf, n, monkeypatch):
    """13 frames: one sub-batch that is no multiple of 8; 24 frames: 2 or 3 sub-batches of 8 / 16 frames"""
    frames = synth.stream(w, h, n, stream_id=500 + n)
    imgs = _device(frames, stride)
    ref, launches, _ = _run(monkeypatch, SERIAL, imgs, w, h, nf)
    assert launches == 1
    for sub in (2, 3, 8):
        got, launches, _ = _run(monkeypatch, _plan(sub), imgs, w, h, nf)
        assert launches == 1 + _sub_batches(n, sub), (sub, launches)   # the level-0 launch, then one per sub-batch: the plan ran
        _assert_same(got, ref, f"{w}x{h} x {n}, {sub} sub-batches")
    if (w, n) in ((64, 24), (320, 24)):
        _oracle(ref, frames, nf, f"{w}x{h}")   # `got` equals `ref` byte for byte


def test_eager_inputs_equal_serial(monkeypatch):
    """inputs whose level 0 is copied (k_pyr_l0* over the whole batch on the main stream, then the same plan)"""
    w, h, nf, n = 320, 240, 500, 24
    frames = synth.stream(w, h, n, stream_id=524)
    rng = np.random.default_rng(7)
    rgb = np.stack([np.clip(frames.astype(np.int32) + rng.integers(-30, 31, frames.shape), 0, 255) for _ in range(3)], 3).astype(np.uint8)
    narrow = synth.stream(63, 64, n, stream_id=525)   # 63 columns: never in place
    for what, imgs, ww, hh, f, fmt, more in (("level 0 not in place", _device(frames), w, h, nf, None, {"ORBX_LEVEL0_INPLACE": "0"}),
                                             ("RGB", _device(rgb), w, h, nf, _capi.FMT_RGB8, {}),
                                             ("63x64", _device(narrow, 64), 63, 64, 200, None, {})):
        ref, launches, _ = _run(monkeypatch, dict(SERIAL, **more), imgs, ww, hh, f, fmt=fmt)
        assert launches == 1
        got, launches, _ = _run(monkeypatch, _plan(3, **more), imgs, ww, hh, f, fmt=fmt)
        assert launches == 4, what
        _assert_same(got, ref, what)


def test_odd_level0_group_count_with_two_groups_per_wave(monkeypatch):
    """k_fast_rows takes FR_GPW = 2 groups per wave when B x (groups of the launch) >= 16384.  128x96 has 9 level-0 groups of 27
    (read from the handle's group table): the fifth wave of a frame's level-0 launch has one group and must not run on into
    level 1's first, whose candidates would then be appended twice.  B = 1824 is the smallest multiple of 16 at which both
    launches of two even sub-batches take two groups per wave.  (The even count: 176 of 526 at 640x480, the next test.)"""
    w, h, nf, l0, total = 128, 96, 300, 9, 27
    n = -(-16384 // min(l0, (total - l0) // 2) // 16) * 16
    assert n == 1824 and n * l0 >= 16384 and (n // 2) % 8 == 0 and (n // 2) * (total - l0) >= 16384
    imgs = _device(synth.stream(w, h, 16, stream_id=530)[np.arange(n) % 16])
    ref, _, groups = _run(monkeypatch, SERIAL, imgs, w, h, nf)
    assert groups == (l0, total)
    got, launches, _ = _run(monkeypatch, _plan(2, ORBX_PLAN_HEAD="0"), imgs, w, h, nf)
    assert launches == 3
    _assert_same(got, ref, f"{w}x{h} x {n}")


def test_vga_256_frames_two_groups_per_wave_default_threshold(monkeypatch):
    """640x480 x 256, the smallest batch that takes the plan by default: 176 level-0 groups of 526 (an even count), both FAST
    launches of both sub-batches at two groups per wave"""
    w, h, nf, n = 640, 480, 1000, 256
    imgs = _device(synth.stream(w, h, 16, stream_id=540)[np.arange(n) % 16])
    ref, _, (l0, total) = _run(monkeypatch, SERIAL, imgs, w, h, nf)
    assert (l0, total) == (176, 526)
    assert n * l0 >= 16384 and (n // 2) * (total - l0) >= 16384
    got, launches, _ = _run(monkeypatch, {"ORBX_PLAN": "fastfirst", "ORBX_PLAN_SUB": "2", "ORBX_PLAN_HEAD": "0"}, imgs, w, h, nf)
    assert launches == 3
    _assert_same(got, ref, "640x480 x 256")


def test_handle_reuse_then_stereo_match(monkeypatch):
    """two calls on one handle with different images: the second equals a fresh handle's (no cursor or status word of the first
    survives the up-front reset); then the batched stereo match on an in-place merged pair batch, which writes level 0 late"""
    import torch
    w, h, nf, B, mb, mbf = 320, 240, 500, 8, 0.11, 47.9
    pairs = [synth.stereo_pair(w, h, stream_id=550 + i) for i in range(B)]
    merged = _device(np.stack([p[0] for p in pairs] + [p[1] for p in pairs]))
    other = _device(synth.stream(w, h, 2 * B, stream_id=560))
    dev = torch.device("cuda", 0)
    outs = []
    for env in (SERIAL, _plan(2)):
        _env(monkeypatch, env)
        ex = ORBextractor(nf, max_batch=2 * B)
        cap = ex.max_keypoints(w, h)
        if env is not SERIAL:   # the first call leaves its cursors and (made-up) status words behind
            first = _buffers(2 * B, cap)
            _extract(ex, other, w, h, first, cap)
            ex.synchronize()
        out = _buffers(2 * B, cap)
        _extract(ex, merged, w, h, out, cap)
        ur = torch.zeros((B, cap), dtype=torch.float32, device=dev); dep = torch.zeros_like(ur)
        nm = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ex.synchronize()
        _capi.check(_capi.lib().orbx_stereo_match_batch_device(
            ex.handle, ex.handle, B, _capi.ptr(out["kps"][:B]), _capi.ptr(out["desc"][:B]), _capi.ptr(out["cnt"][:B]), _capi.ptr(out["kps"][B:]),
            _capi.ptr(out["desc"][B:]), _capi.ptr(out["cnt"][B:]), cap, mb, mbf, _capi.ptr(ur), _capi.ptr(dep), _capi.ptr(nm)))
        ex.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in dict(out, ur=ur, dep=dep, nm=nm).items()})
        ex.close()
    assert outs[0]["nm"].sum() > 0
    _assert_same(outs[1], outs[0], "second call on a used handle + stereo match")


def test_explicit_pipeline_keeps_its_launch_count(monkeypatch):
    """an explicit ORBX_PIPELINE is the sub-batch pipeline as it was, whatever ORBX_PLAN says: one FAST launch per sub-batch"""
    w, h, nf, n = 320, 240, 500, 256
    imgs = _device(synth.stream(w, h, 8, stream_id=570)[np.arange(n) % 8])
    ref, launches, _ = _run(monkeypatch, SERIAL, imgs, w, h, nf)
    assert launches == 1
    for env in ({"ORBX_PIPELINE": "4"}, {"ORBX_PIPELINE": "4", "ORBX_PLAN": "fastfirst"}):
        got, launches, _ = _run(monkeypatch, env, imgs, w, h, nf)
        assert launches == 4, env
        _assert_same(got, ref, f"{env}")
    got, launches, _ = _run(monkeypatch, {}, imgs, w, h, nf)   # the default of a 256-frame batch
    _assert_same(got, ref, "default")
