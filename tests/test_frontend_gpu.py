"""The kernels that turn a camera frame into level 0 and mvKeysUn -- k_pyr_l0_remap (cv::remap of the EuRoC rectification),
k_pyr_l0_color (cvtColor) and k_undistort / k_rgbd (cvUndistortPoints) -- against the independent models of
tests/frontend_model.py on the planted inputs of tests/frontend_scenes.py.  Every comparison is exact: the whole padded level 0
byte for byte, keypoint records and descriptors byte for byte, floats as bit patterns.  No pixel and no keypoint is excluded."""
import ctypes as C

import numpy as np
import pytest

import frontend_model as M
import frontend_scenes as S
import oracle
from orb_slam2_detailed_comments_amd import ORBextractor, synth, _capi

pytestmark = pytest.mark.gpu

GEO = pytest.mark.parametrize("w,h", S.GEOMETRIES, ids=["%dx%d" % g for g in S.GEOMETRIES])
NF = 200
FORMATS = {_capi.FMT_RGB8: (3, True), _capi.FMT_BGR8: (3, False), _capi.FMT_RGBA8: (4, True), _capi.FMT_BGRA8: (4, False)}
SWAPPED = {_capi.FMT_RGB8: _capi.FMT_BGR8, _capi.FMT_BGR8: _capi.FMT_RGB8, _capi.FMT_RGBA8: _capi.FMT_BGRA8, _capi.FMT_BGRA8: _capi.FMT_RGBA8}


@pytest.fixture(autouse=True)
def time_limit():
    """every test here is a GPU step with a limit of its own: a call that does not come back ends the process with a traceback"""
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _layout(frames, row_stride=None, frame_stride=None, offset=0):
    """frames [B, H, W] or [B, H, W, C] -> flat uint8 buffer with frame f, row y at offset + f * frame_stride + y * row_stride;
    every byte that is not a pixel holds 0xEE"""
    b, h = frames.shape[:2]
    row = int(np.prod(frames.shape[2:]))
    row_stride = row_stride or row
    frame_stride = frame_stride or h * row_stride
    assert row_stride >= row and frame_stride >= h * row_stride
    flat = np.full(offset + b * frame_stride + 16, 0xEE, np.uint8)
    for f in range(b):
        for y in range(h):
            at = offset + f * frame_stride + y * row_stride
            flat[at:at + row] = frames[f, y].reshape(-1)
    return flat, row_stride, frame_stride


class Run:
    """one extractor and the output buffers of its calls.  Random-byte frames can overflow a FAST cell's candidate list, which
    the library reports as ORBX_CAPACITY after building the pyramid: the level-0 comparisons accept that status, the keypoint
    comparisons (on synthetic frames) do not."""

    def __init__(self, w, h, max_batch=3, **kw):
        self.ex = ORBextractor(NF, max_batch=max_batch, **kw)
        self.w, self.h, self.cap = w, h, self.ex.max_keypoints(w, h)

    def host(self, flat, b, row_stride, frame_stride, offset=0, strict=False):
        kps = np.zeros((b, self.cap), _capi.KP_DTYPE); desc = np.zeros((b, self.cap, 32), np.uint8); cnt = np.zeros(b, np.int32)
        st = _capi.lib().orbx_extract_batch(self.ex.handle, b, C.c_void_p(flat.ctypes.data + offset), self.w, self.h, row_stride,
                                            frame_stride, _capi.ptr(kps), _capi.ptr(desc), _capi.ptr(cnt), self.cap)
        _capi.check(st, allow=() if strict else (_capi.CAPACITY,))
        return [(kps[i, :cnt[i]].copy(), desc[i, :cnt[i]].copy()) for i in range(b)]

    def device(self, flat, b, row_stride, frame_stride, offset=0):
        """through orbx_extract_batch_device, the image's base pointer `offset` bytes into a device allocation"""
        import torch
        dev = torch.device("cuda", 0)
        owner = torch.from_numpy(flat).to(dev)
        kps = torch.full((b, self.cap * 28), 0xA5, dtype=torch.uint8, device=dev); desc = torch.full((b, self.cap * 32), 0x5A, dtype=torch.uint8, device=dev)
        cnt = torch.full((b,), -3, dtype=torch.int32, device=dev); st = torch.full((b,), -5, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()   # the fills ran on torch's stream, which is not ordered with the handle's
        assert owner.data_ptr() % 4 == 0
        self.ex.extract_batch_device(owner[offset:], b, self.w, self.h, row_stride, frame_stride, kps, desc, cnt, st, self.cap)
        self.ex.synchronize()
        cnt, st = cnt.cpu().numpy(), st.cpu().numpy()
        assert (cnt >= 0).all() and np.isin(st, (_capi.OK, _capi.CAPACITY)).all(), (cnt, st)
        kps, desc = kps.cpu().numpy(), desc.cpu().numpy()
        self._owner = owner
        return [(np.frombuffer(kps[i].tobytes(), _capi.KP_DTYPE)[:cnt[i]], desc[i].reshape(-1, 32)[:cnt[i]]) for i in range(b)], st

    def level0(self, f):
        return self.ex.pyramid_level(0, f)

    def close(self):
        self.ex.close()


def _assert_level0(run, want, what):
    for f, exp in enumerate(want):
        got = run.level0(f)
        assert got.shape == exp.shape, (what, got.shape, exp.shape)
        bad = np.argwhere(got != exp)
        assert len(bad) == 0, f"{what}: frame {f}: {len(bad)} of {exp.size} level-0 bytes differ, first at (row, col) {tuple(bad[0])}: " \
                              f"device {got[tuple(bad[0])]}, model {exp[tuple(bad[0])]}"


# ------------------------------------------------------------------------------------------------------------ rectification
@GEO
def test_rectified_level0_equals_model_on_every_map_scene(w, h):
    """a batch of 3 distinct frames per scene, one handle: every scene replaces the maps of the one before, and switching the
    maps off gives the plain level 0 again"""
    run = Run(w, h)
    frames = S.raw_frames(w, h, 3, seed=w)
    flat, rs, fs = _layout(frames)
    results = {}
    for name, (mx, my, _, _) in S.map_scenes(w, h).items():
        run.ex.set_rectification(mx, my)
        results[name] = run.host(flat, 3, rs, fs)
        _assert_level0(run, [M.pad101(M.remap(fr, mx, my)) for fr in frames], f"{name} {w}x{h}")
    run.ex.set_rectification(None, None)
    plain = run.host(flat, 3, rs, fs)
    _assert_level0(run, [M.pad101(fr) for fr in frames], f"maps off {w}x{h}")
    for (ka, da), (kb, db) in zip(results["identity"], plain):          # the identity map IS plain extraction
        assert ka.tobytes() == kb.tobytes() and da.tobytes() == db.tobytes()
    mx, my, _, _ = S.map_scenes(w, h)["edges"]                          # and on again, a single frame
    run.ex.set_rectification(mx, my)
    flat1, rs, fs = _layout(frames[2:])
    run.host(flat1, 1, rs, fs)
    _assert_level0(run, [M.pad101(M.remap(frames[2], mx, my))], f"edges again, one frame {w}x{h}")
    run.close()


@GEO
def test_rectified_extraction_equals_oracle_on_the_model_rectified_image(w, h):
    """keypoints and descriptors of the planted edge maps: the host entry, then the device entry with rows W + 3 bytes apart
    and the base pointer 1 byte into its allocation"""
    run = Run(w, h)
    frames = synth.stream(w, h, 3, stream_id=700 + w)
    mx, my, _, _ = S.map_scenes(w, h)["edges"]
    run.ex.set_rectification(mx, my)
    rect = [M.remap(fr, mx, my) for fr in frames]
    orc = oracle.OracleExtractor(NF)
    want = []
    for r in rect:
        n, k, d = orc.extract(r, cap=run.cap)
        assert n > 0
        want.append((k, d))
    flat, rs, fs = _layout(frames)
    got = run.host(flat, 3, rs, fs, strict=True)
    _assert_level0(run, [M.pad101(r) for r in rect], f"host entry {w}x{h}")
    for f in range(3):
        assert got[f][0].tobytes() == want[f][0].tobytes() and got[f][1].tobytes() == want[f][1].tobytes(), f"host entry, frame {f}"
    flat, rs, fs = _layout(frames, row_stride=w + 3, offset=1)
    got, st = run.device(flat, 3, rs, fs, offset=1)
    assert not st.any()
    _assert_level0(run, [M.pad101(r) for r in rect], f"device entry, stride {w + 3}, base + 1")
    for f in range(3):
        assert got[f][0].tobytes() == want[f][0].tobytes() and got[f][1].tobytes() == want[f][1].tobytes(), f"device entry, frame {f}"
    run.close()


def test_rectified_level0_in_upstream_mode():
    """ORBX_PYRAMID_UPSTREAM: mvImagePyramid[0] is the un-padded view at origin 19 of the same buffer (three levels: the upstream
    geometry needs 33 pixels at the coarsest)"""
    w, h = S.GEOMETRIES[0]
    run = Run(w, h, pyramid_mode=_capi.PYRAMID_UPSTREAM, nlevels=3)
    frames = S.raw_frames(w, h, 3, seed=11)
    mx, my, _, _ = S.map_scenes(w, h)["edges"]
    run.ex.set_rectification(mx, my)
    flat, rs, fs = _layout(frames)
    run.host(flat, 3, rs, fs)
    _assert_level0(run, [M.remap(fr, mx, my) for fr in frames], "upstream view")
    run.close()


# ------------------------------------------------------------------------------------------------------------ colour input
@GEO
@pytest.mark.parametrize("fmt", list(FORMATS), ids=["rgb", "bgr", "rgba", "bgra"])
def test_colour_level0_equals_model_in_every_layout(w, h, fmt):
    nch, rgb = FORMATS[fmt]
    r_off, b_off = (0, 2) if rgb else (2, 0)
    run = Run(w, h)
    run.ex.set_input_format(fmt)
    frames, masks = S.colour_frames(w, h, nch, 3, seed=w + fmt, rgb=rgb)
    want = [M.pad101(M.cvt_gray(fr, r_off, b_off)) for fr in frames]
    row = w * nch
    # host entry: contiguous, rows W * nch + 5 bytes apart, frames with a gap between them; batches of 3 and 1
    for what, kw in (("contiguous", {}), ("row stride + 5", dict(row_stride=row + 5)), ("frame gap", dict(frame_stride=h * row + 77)),
                     ("padded rows and frame gap", dict(row_stride=row + 5, frame_stride=h * (row + 5) + 31))):
        flat, rs, fs = _layout(frames, **kw)
        run.host(flat, 3, rs, fs)
        _assert_level0(run, want, f"host, {what}")
    flat, rs, fs = _layout(frames[1:2], row_stride=row + 5)
    run.host(flat, 1, rs, fs)
    _assert_level0(run, want[1:2], "host, one frame")
    # device entry: the base pointer 1, 2 and 3 bytes into the allocation
    for off, kw, b in ((1, {}, 3), (2, dict(row_stride=row + 5), 3), (3, dict(frame_stride=h * row + 77), 3), (3, {}, 1)):
        flat, rs, fs = _layout(frames[:b], offset=off, **kw)
        run.device(flat, b, rs, fs, offset=off)
        _assert_level0(run, want[:b], f"device, base + {off}, {kw}, {b} frame(s)")
    # planted check that a swap of R and B is visible: the other order on the same bytes
    run.ex.set_input_format(SWAPPED[fmt])
    flat, rs, fs = _layout(frames)
    run.host(flat, 3, rs, fs)
    swapped = [M.pad101(M.cvt_gray(fr, b_off, r_off)) for fr in frames]
    _assert_level0(run, swapped, "R and B swapped")
    for f in range(3):
        a, s = want[f][M.EDGE:-M.EDGE, M.EDGE:-M.EDGE].astype(int), run.level0(f)[M.EDGE:-M.EDGE, M.EDGE:-M.EDGE].astype(int)
        for c in ("pure_r", "pure_b"):
            assert (np.abs(a - s)[masks[c][f]] == 47).all(), c        # 76 against 29
        for c in ("pure_g", "black", "white"):
            assert (a == s)[masks[c][f]].all(), c
        assert (a[masks["white"][f]] == 255).all() and (a[masks["black"][f]] == 0).all()
    run.close()


# ------------------------------------------------------------------------------------------------------------ undistortion
@pytest.fixture(scope="module")
def ex():
    e = ORBextractor(NF, max_batch=4)
    yield e
    e.close()


@pytest.mark.parametrize("model", list(S.DIST_MODELS))
def test_undistort_host_entry_and_image_bounds_equal_model(ex, model):
    L, P = _capi.lib(), _capi.ptr
    D = np.array(S.DIST_MODELS[model], np.float32); k4 = np.array(S.TUM1_K, np.float32)
    for n in S.COUNTS:
        k, _ = S.keypoints(n, _capi.KP_DTYPE, seed=n)
        out = np.zeros(n, _capi.KP_DTYPE)
        _capi.check(L.orbx_undistort_keypoints(ex.handle, P(k), n, P(k4), P(D), len(D), P(out)))
        assert out.tobytes() == M.undistort_keypoints(k, S.TUM1_K, D).tobytes(), (model, n)
        if model == "prism_14_zero_tilt":
            assert out.tobytes() == M.undistort_keypoints(k, S.TUM1_K, S.D12).tobytes()
    b = np.zeros(4, np.float32)
    _capi.check(L.orbx_image_bounds(ex.handle, S.IMAGE_WH[0], S.IMAGE_WH[1], P(k4), P(D), len(D), P(b)))
    assert np.array_equal(b.view(np.uint32), M.image_bounds(*S.IMAGE_WH, S.TUM1_K, D).view(np.uint32)), (b, model)


def _device_batch():
    """four frames of `cap` records, counts 1, 255, 256, 257: (keys [B, cap], counts)"""
    cap = 300
    keys = np.stack([S.keypoints(cap, _capi.KP_DTYPE, seed=40 + f)[0] for f in range(len(S.COUNTS))])
    return keys, np.array(S.COUNTS, np.int32), cap


@pytest.mark.parametrize("model", list(S.DIST_MODELS))
def test_undistort_device_entry_with_per_frame_counts_equals_model(ex, model):
    import torch
    L, P = _capi.lib(), _capi.ptr
    D = np.array(S.DIST_MODELS[model], np.float32); k4 = np.array(S.TUM1_K, np.float32)
    keys, counts, cap = _device_batch()
    B = len(counts)
    dev = torch.device("cuda", 0)
    d_k = torch.from_numpy(keys.view(np.uint8).reshape(B, cap * 28)).to(dev); d_c = torch.from_numpy(counts).to(dev)
    d_o = torch.full((B, cap * 28), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    _capi.check(L.orbx_undistort_keypoints_device(ex.handle, B, P(d_k), P(d_c), cap, P(k4), P(D), len(D), P(d_o)))
    ex.synchronize()
    out = d_o.cpu().numpy()
    for f in range(B):
        n = int(counts[f])
        assert out[f, :n * 28].tobytes() == M.undistort_keypoints(keys[f, :n], S.TUM1_K, D).tobytes(), (model, f)
        assert (out[f, n * 28:] == 0xA5).all(), f"records beyond counts[{f}] were written"


def test_rgbd_entry_writes_the_records_of_k_undistort():
    """orbx_rgbd_depth_device with the 8-term model: mvKeysUn as k_undistort writes it, records beyond the counts untouched"""
    import torch
    L, P = _capi.lib(), _capi.ptr
    ex = ORBextractor(NF, max_batch=4)
    D = np.array(S.D8, np.float32); k4 = np.array(S.TUM1_K, np.float32)
    keys, counts, cap = _device_batch()
    B = len(counts); w, h = S.IMAGE_WH
    dev = torch.device("cuda", 0)
    d_k = torch.from_numpy(keys.view(np.uint8).reshape(B, cap * 28)).to(dev); d_c = torch.from_numpy(counts).to(dev)
    d_u = torch.full((B, cap * 28), 0xA5, dtype=torch.uint8, device=dev); d_r = torch.full((B, cap * 28), 0xA5, dtype=torch.uint8, device=dev)
    depth = torch.full((B, h, w), 5000, dtype=torch.int16, device=dev)
    ur = torch.full((B, cap), -7.0, dtype=torch.float32, device=dev); dp = torch.full((B, cap), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    _capi.check(L.orbx_undistort_keypoints_device(ex.handle, B, P(d_k), P(d_c), cap, P(k4), P(D), len(D), P(d_u)))
    ex.rgbd_depth_device(B, d_k, d_c, cap, S.TUM1_K, D, depth, _capi.DEPTH_U16, w, h, 2 * w, 2 * w * h, 1.0 / 5000.0, 40.0, d_r, ur, dp)
    ex.synchronize()
    a, b = d_u.cpu().numpy(), d_r.cpu().numpy()
    assert np.array_equal(a, b)
    ur, dp = ur.cpu().numpy(), dp.cpu().numpy()
    for f in range(B):
        n = int(counts[f])
        assert b[f, :n * 28].tobytes() == M.undistort_keypoints(keys[f, :n], S.TUM1_K, D).tobytes()
        assert (b[f, n * 28:] == 0xA5).all() and (ur[f, n:] == -7.0).all() and (dp[f, n:] == -7.0).all()
        assert (dp[f, :n] != -7.0).all() and (n == 1 or (dp[f, :n] > 0).any())      # (the single record lies outside the image)
    ex.close()
