"""The sub-batch pipeline of the batched extraction (csrc/orbx_extract.cpp run_chunk, ORBX_PIPELINE): the pyramids of the sub-batches
run on the handle's side stream while FAST / quadtree / descriptors of the previous sub-batch run on its main stream.  It changes
launch order and residency only: every output must be byte-identical to the serial sequence (ORBX_PIPELINE=0) -- keypoints,
descriptors, counts, status words and the t vs t-1 match of the whole batch, seams between sub-batches included."""
import numpy as np
import pytest
from orb_slam2_detailed_comments_amd import ORBextractor, synth, _capi

pytestmark = pytest.mark.gpu

W, H, NF = 640, 480, 1000


def _frames(w, h, n, base, sid, nch=1):
    """n frames cycling through `base` distinct synthetic frames (device tensor); nch > 1: colour frames derived from them"""
    import torch
    g = synth.stream(w, h, base, stream_id=sid)
    if nch > 1:
        rng = np.random.default_rng(sid)
        g = np.stack([np.clip(g.astype(np.int32) + rng.integers(-30, 31, g.shape), 0, 255) for _ in range(nch)], 3).astype(np.uint8)
    idx = np.arange(n) % base
    return torch.from_numpy(np.ascontiguousarray(g[idx])).to(torch.device("cuda", 0))


def _run(monkeypatch, env, imgs, n, w, h, nf=NF, fmt=None, maps=None, match=True):
    """one fresh handle under `env`, one device-pointer call over the n frames, then frame t matched against t-1 on the device"""
    import torch
    for k in ("ORBX_PIPELINE", "ORBX_PIPELINE_HEAD", "ORBX_FAST_ROOM", "ORBX_FORK_LEVEL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ex = ORBextractor(nf, max_batch=n)
    if fmt is not None:
        ex.set_input_format(fmt)
    if maps is not None:
        ex.set_rectification(*maps)
    cap = ex.max_keypoints(w, h)
    dev = torch.device("cuda", 0)
    kps = torch.full((n, cap * 28), 0xA5, dtype=torch.uint8, device=dev); desc = torch.full((n, cap * 32), 0x5A, dtype=torch.uint8, device=dev)
    cnt = torch.full((n,), -3, dtype=torch.int32, device=dev); st = torch.full((n,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()   # the fills ran on torch's stream, which is not ordered with the handle's
    ex.extract_batch_device(imgs, n, w, h, imgs.stride(1), imgs.stride(0), kps, desc, cnt, st, cap)
    out = dict(kps=kps, desc=desc, cnt=cnt, st=st)
    if match:
        ex.synchronize()
        tr_desc = torch.roll(desc, 1, 0).contiguous(); tr_cnt = torch.roll(cnt, 1, 0).contiguous()
        mi = torch.full((n, cap), -7, dtype=torch.int32, device=dev); mb = torch.zeros_like(mi); ms = torch.zeros_like(mi)
        torch.cuda.synchronize()
        _capi.check(_capi.lib().orbx_match_bruteforce_device(ex.handle, n, _capi.ptr(desc), _capi.ptr(cnt), cap * 32, _capi.ptr(tr_desc),
                                                             _capi.ptr(tr_cnt), cap * 32, _capi.ptr(mi), _capi.ptr(mb), _capi.ptr(ms), cap))
        out.update(mi=mi, mb=mb, ms=ms)
    ex.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    ex.close()
    return res


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    assert (a["cnt"] > 0).all(), what
    assert not a["st"].any(), what
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs from the serial sequence"


@pytest.mark.parametrize("n", [1, 7, 255, 256, 1024])
def test_pipelined_equals_serial_grey(n, monkeypatch):
    imgs = _frames(W, H, n, min(n, 24), sid=300)
    ref = _run(monkeypatch, {"ORBX_PIPELINE": "0"}, imgs, n, W, H)
    _assert_same(_run(monkeypatch, {}, imgs, n, W, H), ref, f"default, {n} frames")
    if n >= 256:   # even and uneven (small head) splits, every sub-batch count, and the pipeline without the FAST wave cap
        for env in ({"ORBX_PIPELINE": "2"}, {"ORBX_PIPELINE": "8"}, {"ORBX_PIPELINE": "3", "ORBX_PIPELINE_HEAD": "0"},
                    {"ORBX_PIPELINE": "8", "ORBX_PIPELINE_HEAD": "1"}, {"ORBX_PIPELINE": "4", "ORBX_FAST_ROOM": "0"}):
            _assert_same(_run(monkeypatch, env, imgs, n, W, H), ref, f"{env}, {n} frames")


@pytest.mark.parametrize("fmt,nch", [(_capi.FMT_RGB8, 3), (_capi.FMT_BGRA8, 4)])
def test_pipelined_equals_serial_colour(fmt, nch, monkeypatch):
    n = 300
    imgs = _frames(W, H, n, 12, sid=310, nch=nch)
    ref = _run(monkeypatch, {"ORBX_PIPELINE": "0"}, imgs, n, W, H, fmt=fmt)
    _assert_same(_run(monkeypatch, {}, imgs, n, W, H, fmt=fmt), ref, f"colour {fmt}")


def test_pipelined_equals_serial_rectified(monkeypatch):
    w, h, nf, n = 752, 480, 1200, 264
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = (xx - w / 2 - 3.3) / (0.6 * w), (yy - h / 2 + 2.1) / (0.6 * w)
    r2 = x * x + y * y
    k = 1 - 0.28 * r2 + 0.07 * r2 * r2
    maps = ((x * k * 0.6 * w + w / 2 + 3.3).astype(np.float32), (y * k * 0.6 * w + h / 2 - 2.1).astype(np.float32))
    imgs = _frames(w, h, n, 11, sid=320)
    ref = _run(monkeypatch, {"ORBX_PIPELINE": "0"}, imgs, n, w, h, nf=nf, maps=maps)
    _assert_same(_run(monkeypatch, {}, imgs, n, w, h, nf=nf, maps=maps), ref, "rectified")


def test_pipelined_merged_stereo_batch(monkeypatch):
    """both eyes of B pairs in one extractor batch of 2B images, then the batched stereo match on the same handle (which reads
    the right pyramids): uRight / depth / match counts identical to the serial sequence"""
    import torch
    w, h, nf, B, mb, mbf = 752, 480, 1200, 160, 0.11, 47.9
    pairs = [synth.stereo_pair(w, h, stream_id=330 + i) for i in range(8)]
    dev = torch.device("cuda", 0)
    imgs = torch.from_numpy(np.stack([pairs[i % 8][0] for i in range(B)] + [pairs[i % 8][1] for i in range(B)])).to(dev)
    outs = []
    for env in ({"ORBX_PIPELINE": "0"}, {}, {"ORBX_PIPELINE": "8"}):
        for k in ("ORBX_PIPELINE", "ORBX_PIPELINE_HEAD", "ORBX_FAST_ROOM", "ORBX_FORK_LEVEL"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ex = ORBextractor(nf, max_batch=2 * B)
        cap = ex.max_keypoints(w, h)
        kps = torch.zeros((2 * B, cap * 28), dtype=torch.uint8, device=dev); desc = torch.zeros((2 * B, cap * 32), dtype=torch.uint8, device=dev)
        cnt = torch.zeros(2 * B, dtype=torch.int32, device=dev); st = torch.full((2 * B,), -5, dtype=torch.int32, device=dev)
        ur = torch.zeros((B, cap), dtype=torch.float32, device=dev); dep = torch.zeros_like(ur)
        nm = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ex.extract_batch_device(imgs, 2 * B, w, h, w, w * h, kps, desc, cnt, st, cap)
        _capi.check(_capi.lib().orbx_stereo_match_batch_device(
            ex.handle, ex.handle, B, _capi.ptr(kps[:B]), _capi.ptr(desc[:B]), _capi.ptr(cnt[:B]), _capi.ptr(kps[B:]),
            _capi.ptr(desc[B:]), _capi.ptr(cnt[B:]), cap, mb, mbf, _capi.ptr(ur), _capi.ptr(dep), _capi.ptr(nm)))
        ex.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in dict(kps=kps, desc=desc, cnt=cnt, st=st, ur=ur, dep=dep, nm=nm).items()})
        ex.close()
    assert (outs[0]["nm"] > 20).all()
    for o, what in zip(outs[1:], ("default", "8 sub-batches")):
        _assert_same(o, outs[0], f"merged stereo, {what}")


def test_fork_level_selects_the_serial_sub_batch_sequence(monkeypatch):
    """ORBX_FORK_LEVEL > 0 and the pipeline exclude each other (both use the side stream): with both set, the fork runs, and
    the outputs still equal the plain serial sequence"""
    n = 256
    imgs = _frames(W, H, n, 16, sid=340)
    ref = _run(monkeypatch, {"ORBX_PIPELINE": "0"}, imgs, n, W, H)
    for env in ({"ORBX_FORK_LEVEL": "3"}, {"ORBX_FORK_LEVEL": "4", "ORBX_PIPELINE": "4"}):
        _assert_same(_run(monkeypatch, env, imgs, n, W, H), ref, f"{env}")


def test_pipelined_host_entry_and_profiled_calls(monkeypatch):
    """the host-buffer entry (one chunk of >= 256 frames goes through the pipeline) and a call with every kernel profiled
    (the calibration pass of bench.py --full, which runs the serial sequence) against the serial sequence"""
    n = 256
    frames = synth.stream(W, H, 16, stream_id=350)[np.arange(n) % 16]
    outs = []
    k_fast = _capi.K_NAMES.index("k_fast_rows")
    for env, mask in (({"ORBX_PIPELINE": "0"}, 0), ({}, 0), ({"ORBX_PIPELINE": "4"}, 0x1ff), ({"ORBX_PIPELINE": "4"}, 1 << k_fast)):
        for k in ("ORBX_PIPELINE", "ORBX_PIPELINE_HEAD", "ORBX_FAST_ROOM", "ORBX_FORK_LEVEL"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ex = ORBextractor(NF, max_batch=n)
        ex.profile_enable(mask)
        res = ex.extract_batch(frames)
        if mask:   # every kernel profiled: one launch each (serial); FAST alone: one launch per sub-batch (pipelined)
            prof = ex.profile_read()
            assert prof["k_fast_rows"][1] == (1 if mask == 0x1ff else 4) and prof["k_fast_rows"][0] > 0
        outs.append(b"".join(k.tobytes() + d.tobytes() for k, d in res))
        ex.close()
    assert all(o == outs[0] for o in outs[1:])
