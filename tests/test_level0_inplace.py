"""In-place level 0 (csrc/orbx_inplace.h, run_chunk): grey batches of the device entry read level 0 from the caller's image --
k_pyr_l0 is not launched, its padded copy is only written when somebody asks for it (ensure_level0).  The mode changes where
bytes are read from, nothing else: against ORBX_LEVEL0_INPLACE=0 on a fresh handle every keypoint, descriptor, count, status
word and every pyramid level must be equal byte for byte, and frame 0 and the last frame must equal the oracle."""
import numpy as np
import pytest
import oracle
from orb_slam2_detailed_comments_amd import ORBextractor, synth, _capi

pytestmark = pytest.mark.gpu

L0_BIT = 1 << _capi.K_NAMES.index("k_pyr_l0")


def _device_frames(frames, stride, offset=0):
    """frames [B,H,W] -> (owner tensor, tensor view whose data pointer is base + offset), rows `stride` bytes apart, the bytes
    between W and stride filled with a value no frame row ends on"""
    import torch
    b, h, w = frames.shape
    host = np.full((b, h, stride), 0xEE, np.uint8)
    host[:, :, :w] = frames
    flat = torch.zeros(b * h * stride + 16, dtype=torch.uint8, device=torch.device("cuda", 0))
    flat[offset:offset + b * h * stride] = torch.from_numpy(host.reshape(-1)).to(flat.device)
    return flat, flat[offset:offset + b * h * stride]


def _run(monkeypatch, inplace, frames, stride=None, offset=0, nf=1000, levels_of=None):
    """fresh handle, one device-pointer call; returns outputs, the pyramid levels of the frames `levels_of`, and how many
    k_pyr_l0 launches the extraction itself made (0 = it ran in place)"""
    import torch
    b, h, w = frames.shape
    stride = stride or w
    monkeypatch.delenv("ORBX_LEVEL0_INPLACE", raising=False)
    if not inplace:
        monkeypatch.setenv("ORBX_LEVEL0_INPLACE", "0")
    ex = ORBextractor(nf, max_batch=b)
    ex.profile_enable(L0_BIT)   # one bit: the launch sequence stays the default one
    cap = ex.max_keypoints(w, h)
    dev = torch.device("cuda", 0)
    owner, imgs = _device_frames(frames, stride, offset)
    kps = torch.full((b, cap * 28), 0xA5, dtype=torch.uint8, device=dev); desc = torch.full((b, cap * 32), 0x5A, dtype=torch.uint8, device=dev)
    cnt = torch.full((b,), -3, dtype=torch.int32, device=dev); st = torch.full((b,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ex.extract_batch_device(imgs, b, w, h, stride, h * stride, kps, desc, cnt, st, cap)
    ex.synchronize()
    l0_launches = ex.profile_read()["k_pyr_l0"][1]
    out = {k: v.cpu().numpy() for k, v in dict(kps=kps, desc=desc, cnt=cnt, st=st).items()}
    frames_of = range(b) if levels_of is None else levels_of
    out["pyr"] = {(l, f): ex.pyramid_level(l, f) for f in frames_of for l in range(8)}
    del owner
    return ex, out, l0_launches


def _same(a, b, what):
    for k in ("cnt", "st", "kps", "desc"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"
    assert (a["cnt"] > 0).all() and not a["st"].any(), what
    assert a["pyr"].keys() == b["pyr"].keys()
    for key in a["pyr"]:
        assert np.array_equal(a["pyr"][key], b["pyr"][key]), f"{what}: pyramid level {key[0]} of frame {key[1]} differs"


def _oracle(out, frames, nf, what):
    cap = out["kps"].shape[1] // 28
    for f in (0, len(frames) - 1):
        orc = oracle.OracleExtractor(nf)
        n, k, d = orc.extract(np.ascontiguousarray(frames[f]), cap=cap)
        assert n == int(out["cnt"][f]), (what, f)
        assert out["kps"][f][:n * 28].tobytes() == k.tobytes(), f"{what}: keypoints of frame {f} differ from the oracle"
        assert out["desc"][f][:n * 32].tobytes() == d.tobytes(), f"{what}: descriptors of frame {f} differ from the oracle"
        for l in range(8):
            assert np.array_equal(out["pyr"][(l, f)], orc.level_image(l)), f"{what}: level {l} of frame {f} differs from the oracle"


def _ab(monkeypatch, frames, expect_inplace, what, stride=None, offset=0, nf=1000, levels_of=None):
    exa, a, la = _run(monkeypatch, True, frames, stride, offset, nf, levels_of)
    exb, b, lb = _run(monkeypatch, False, frames, stride, offset, nf, levels_of)
    assert lb > 0, f"{what}: the eager run did not launch k_pyr_l0"
    assert (la == 0) == expect_inplace, f"{what}: k_pyr_l0 launches of the default run = {la}"
    _same(a, b, what)
    _oracle(a, frames, nf, what)
    exa.close(); exb.close()


@pytest.mark.parametrize("B", [3, 9])
def test_vga_batches(monkeypatch, B):
    _ab(monkeypatch, synth.stream(640, 480, B, stream_id=400 + B), True, f"640x480 x {B}")


@pytest.mark.parametrize("w,h,stride", [(639, 479, 640), (97, 75, 100)])
def test_odd_sizes_with_row_padding(monkeypatch, w, h, stride):
    _ab(monkeypatch, synth.stream(w, h, 3, stream_id=410), True, f"{w}x{h} stride {stride}", stride=stride)


def test_smallest_geometry_and_one_below(monkeypatch):
    """64 x 64 is the smallest image the mode takes (ORBX_IP_MIN_W / ORBX_IP_MIN_H); 63 columns fall back to k_pyr_l0"""
    _ab(monkeypatch, synth.stream(64, 64, 8, stream_id=420), True, "64x64", nf=200, levels_of=(0, 7))
    _ab(monkeypatch, synth.stream(63, 64, 8, stream_id=421), False, "63x64", stride=64, nf=200, levels_of=(0, 7))


def test_unaligned_input_falls_back(monkeypatch):
    fr = synth.stream(640, 480, 8, stream_id=430)
    _ab(monkeypatch, fr, False, "stride 641", stride=641, levels_of=(0, 7))
    _ab(monkeypatch, fr, False, "base + 1", offset=1, levels_of=(0, 7))


def test_pipelined_sequence_runs_in_place(monkeypatch):
    """256 frames: the sub-batch pipeline (every sub-batch's level-1 launch resets its own frames' status / cursors)"""
    base = synth.stream(320, 240, 8, stream_id=440)
    frames = base[np.arange(256) % 8]
    _ab(monkeypatch, frames, True, "320x240 x 256", nf=500, levels_of=(0, 255))


def test_ring_columns_and_rows_matter(monkeypatch):
    """bright one-pixel frames on rows / columns 0..2 and their mirror images: what the reflect-101 ring is made of"""
    fr = synth.stream(320, 240, 8, stream_id=450).copy()
    for k, v in enumerate((255, 140, 230)):
        fr[:, k, k:320 - k] = v; fr[:, 239 - k, k:320 - k] = v
        fr[:, k:240 - k, k] = v; fr[:, k:240 - k, 319 - k] = v
    _ab(monkeypatch, fr, True, "ring image", nf=500, levels_of=(0, 7))


def test_merged_stereo_pair_builds_level0_late(monkeypatch):
    """orbx_stereo_match_batch_device reads the padded level 0 of both eyes: an in-place batch writes it late, the results equal
    the eager ones, and the handle's next batch is eager again"""
    import torch
    w, h, nf, B, mb, mbf = 320, 240, 500, 8, 0.11, 47.9
    pairs = [synth.stereo_pair(w, h, stream_id=460 + i) for i in range(B)]
    dev = torch.device("cuda", 0)
    imgs = torch.from_numpy(np.stack([p[0] for p in pairs] + [p[1] for p in pairs])).to(dev)
    outs, launches = [], []
    for inplace in (True, False):
        monkeypatch.delenv("ORBX_LEVEL0_INPLACE", raising=False)
        if not inplace:
            monkeypatch.setenv("ORBX_LEVEL0_INPLACE", "0")
        ex = ORBextractor(nf, max_batch=2 * B)
        ex.profile_enable(L0_BIT)
        cap = ex.max_keypoints(w, h)
        kps = torch.zeros((2 * B, cap * 28), dtype=torch.uint8, device=dev); desc = torch.zeros((2 * B, cap * 32), dtype=torch.uint8, device=dev)
        cnt = torch.zeros(2 * B, dtype=torch.int32, device=dev); st = torch.full((2 * B,), -5, dtype=torch.int32, device=dev)
        ur = torch.zeros((B, cap), dtype=torch.float32, device=dev); dep = torch.zeros_like(ur)
        nm = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        seq = []
        for rep in range(2):
            ex.extract_batch_device(imgs, 2 * B, w, h, w, w * h, kps, desc, cnt, st, cap)
            ex.synchronize()
            seq.append(ex.profile_read()["k_pyr_l0"][1])
            _capi.check(_capi.lib().orbx_stereo_match_batch_device(
                ex.handle, ex.handle, B, _capi.ptr(kps[:B]), _capi.ptr(desc[:B]), _capi.ptr(cnt[:B]), _capi.ptr(kps[B:]),
                _capi.ptr(desc[B:]), _capi.ptr(cnt[B:]), cap, mb, mbf, _capi.ptr(ur), _capi.ptr(dep), _capi.ptr(nm)))
            ex.synchronize()
            seq.append(ex.profile_read()["k_pyr_l0"][1])
        launches.append(seq)
        outs.append({k: v.cpu().numpy() for k, v in dict(kps=kps, desc=desc, cnt=cnt, st=st, ur=ur, dep=dep, nm=nm).items()})
        ex.close()
    assert launches[0] == [0, 1, 1, 0], launches[0]   # in place, late copy for the match, then eager
    assert launches[1] == [1, 0, 1, 0], launches[1]
    assert outs[0]["nm"].sum() > 0 and not outs[0]["st"].any()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), f"merged stereo: {k} differs"
