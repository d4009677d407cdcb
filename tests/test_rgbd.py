"""RGB-D Frame (reference src/Frame.cc:237-321): Frame::ComputeStereoFromRGBD (:1179-1226) after Tracking::GrabImageRGBD's
depth conversion (src/Tracking.cc:327-332), with the F7 rule: a depth sample past the image's memory
gives no depth.  k_rgbd fuses it with k_undistort.

CPU part: tests/rgbd_model.py against hand-worked cases (factor rule, the three conversion branches, truncation, row wrap, the
F7 boundary, the strided-f32 gap), the F7 counts of the committed golden keypoints, argument validation on a host-only handle,
the code object (no scratch, correctly rounded division) and the compat body under -Wall -Werror.  GPU part: bit-exact
mvKeysUn / mvuRight / mvDepth against the oracle plus the model, agreement of the device-resident, host-fed and single-frame
paths (chunking, page-locked depth, both ORBX_RGBD_DEPTH modes), adversarial values, mono outputs unchanged by interleaved
RGB-D calls, the compat body through its stand-ins, and a seeded soak."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import rgbd_model as M
from orb_slam2_detailed_comments_amd import ORBextractor, OrbxError, Frame, depth_map_factor, synth, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "lib")
HERE = os.path.join(ROOT, "tests", "compat_rgbd")
TUM_K = (517.306408, 516.469215, 318.643040, 255.313989)                  # Examples/RGB-D/TUM1.yaml
TUM_D = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
TUM_BF = 40.0
NAMES = ("orbx_rgbd_depth_device", "orbx_rgbd_depth", "orbx_extract_rgbd_batch")


def keys(xs, ys):
    k = np.zeros(len(xs), _capi.KP_DTYPE)
    k["x"] = np.asarray(xs, np.float32); k["y"] = np.asarray(ys, np.float32)
    k["size"] = 31; k["octave"] = 0; k["class_id"] = -1
    return k


def _status(fn):
    with pytest.raises(OrbxError) as e:
        fn()
    return e.value.status


# ----------------------------------------------------------------------------------------------- CPU: the model
def test_depth_map_factor_rule():
    for f in (5000.0, 1000.0, 1.0, -5000.0, 3.0, 1e-5, 2e-5, 0.0, 1e-6, -1e-6, 9.99e-6):
        want = M.depth_map_factor(f)
        got = depth_map_factor(f)
        assert got.dtype == np.float32 and M.bits(got) == M.bits(want), f
    assert depth_map_factor(5000.0) == np.float32(1) / np.float32(5000)
    # |f| < 1e-5 goes to 1: float32(1e-5) = 9.99999975e-06 is below the double 1e-5
    assert depth_map_factor(0.0) == 1 and depth_map_factor(1e-6) == 1 and depth_map_factor(1e-5) == 1
    assert depth_map_factor(2e-5) == np.float32(1) / np.float32(2e-5)


def test_conversion_branches():
    raw = np.array([[0, 1, 5000], [65535, 7, 2]], np.uint16)
    img, pitch, limit = M.float_image(raw, np.float32(2e-4))
    assert pitch == 12 and limit == 24
    assert M.bits(img).tolist() == M.bits(raw.reshape(-1).astype(np.float32) * np.float32(2e-4)).tolist()
    f = np.array([[1.0, -2.0, np.nan], [np.inf, 0.5, 3.0]], np.float32)
    for s, conv in ((1.0, False), (1.0 + 1e-6, False), (1.5, True), (np.float32(2e-4), True)):
        assert M.converts_f32(s) == conv, s
        img, pitch, _ = M.float_image(f, s)
        want = f.reshape(-1) * np.float32(s) if conv else f.reshape(-1)
        assert M.bits(img).tolist() == M.bits(want).tolist(), s   # raw values when not converted, even for scale != 1


def test_truncation_row_wrap_and_f7_boundary():
    W, H = 5, 4
    raw = np.arange(1, W * H + 1, dtype=np.uint16).reshape(H, W)
    s = np.float32(1)
    # x.9999 truncates; u >= W wraps into the next row; the last pixel is the last sample inside
    xs = [1.9999, W + 2.0, W - 1 + 0.5, float(W), 0.0, -0.5, np.nan, np.inf, 3e9, 2.0]
    ys = [0.9999, 1.0, H - 1.0, H - 1.0, H - 0.0001, 0.0, 0.0, 0.0, 0.0, 1e10]
    ur, dp = M.rgbd_depth(np.float32(xs), np.float32(ys), np.float32(xs), raw, s, 10.0)
    assert dp[0] == 2                     # (0, 1)
    assert dp[1] == raw[2, 2]             # (1, W + 2) wraps to (2, 2)
    assert dp[2] == raw[H - 1, W - 1]     # o + 4 == limit: inside
    assert dp[3] == -1                    # o + 4 == limit + 4: F7
    assert dp[4] == raw[H - 1, 0]         # y truncates to H - 1
    assert (dp[5:] == -1).all() and (ur[5:] == -1).all()   # negative, NaN, inf, too large
    assert ur[0] == np.float32(1.9999) - np.float32(10) / np.float32(2)


def test_strided_f32_gap_and_boundary():
    W, H, P = 3, 3, 5                     # 5 floats per row: 2 gap floats
    wide = np.arange(1, H * P + 1, dtype=np.float32).reshape(H, P)
    view = wide[:, :W]
    img, pitch, limit = M.float_image(view, 2.0)
    assert pitch == 20 and limit == 2 * 20 + 12
    xs = np.float32([3.0, 4.0, 2.0, 3.0, 5.0])
    ys = np.float32([0.0, 1.0, 2.0, 2.0, 0.0])
    ur, dp = M.rgbd_depth(xs, ys, xs, view, 2.0, 1.0)
    assert dp[0] == wide[0, 3]            # gap: raw, unscaled
    assert dp[1] == wide[1, 4]
    assert dp[2] == 2 * wide[2, 2]        # last sample inside, scaled
    assert dp[3] == -1                    # past (H - 1) * pitch + 4 * W: F7 (the gap after the last row is not the image's)
    assert dp[4] == 2 * wide[1, 0]        # u = 5 wraps into row 1, scaled
    assert M.f7_counts(xs, ys, W, H, pitch)[1] == 1


def test_f7_counts_on_golden_keypoints():
    """the committed golden extractions: 41/236, 66/204 and 16/76 keypoints sample past the depth buffer"""
    want = {"s160x120": (236, 41), "s200x96": (204, 66), "s97x131": (76, 16)}
    for name, (n, past) in want.items():
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        k = z["kps_fma"].view(_capi.KP_DTYPE).reshape(-1)
        H, W = z["image"].shape
        assert len(k) == n and M.f7_counts(k["x"], k["y"], W, H)[1] == past, name
        assert k["x"].min() >= 19 and k["y"].min() >= 19          # padded coordinates


def test_synthetic_depth_is_seeded_and_has_holes():
    a = synth.depth_stream(160, 120, 3, stream_id=4)
    b = synth.depth_stream(160, 120, 3, stream_id=4)
    assert a.dtype == np.uint16 and a.shape == (3, 120, 160) and np.array_equal(a, b)
    holes = (a == 0).mean()
    assert 0.03 < holes < 0.2 and a.max() < 65535 and a[a > 0].min() >= 2500
    f = synth.depth_stream(160, 120, 2, stream_id=4, fmt="f32")
    assert f.dtype == np.float32 and 0.03 < np.isnan(f).mean() < 0.2


# ----------------------------------------------------------------------------------------------- CPU: ABI
def test_symbols_declared_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "orbx.h")).read()
    assert "ORBX_DEPTH_U16 = 0, ORBX_DEPTH_F32 = 1" in header
    L = _capi.lib()
    for name in NAMES:
        assert f"orbx_status {name}(" in header and name in _capi.SYMBOLS and hasattr(L, name)


def test_host_only_validation(built_lib):
    L = _capi.lib()
    ex = ORBextractor(1000, device=-2)
    h = ex.handle
    k = keys([30.0], [30.0])
    dep = np.zeros((48, 64), np.uint16); depf = np.zeros((48, 64), np.float32)
    ur = np.zeros(4, np.float32); dp = np.zeros(4, np.float32)
    P = _capi.ptr
    one = lambda fmt, d, w, hh, st, kk=k, n=1, o1=ur, o2=dp: L.orbx_rgbd_depth(h, P(kk), P(kk), n, P(d) if d is not None else None,
                                                                               fmt, w, hh, st, 1.0, 40.0, P(o1), P(o2))
    B = _capi.BAD_ARGUMENT
    assert one(2, dep, 64, 48, 128) == B                  # format
    assert one(-1, dep, 64, 48, 128) == B
    assert one(0, dep, 64, 48, 126) == B                  # stride < W * 2
    assert one(1, depf, 64, 48, 255) == B                 # stride < W * 4
    assert one(1, depf, 32, 48, 130) == B                 # stride not a multiple of 4
    assert one(0, dep, 64, 48, 131) == B                  # odd stride for u16
    assert one(0, None, 64, 48, 128) == B                 # null depth
    assert one(0, dep, 0, 48, 128) == B and one(0, dep, 64, 0, 128) == B
    assert one(0, dep, 64, 48, 128, n=-1) == B
    assert one(0, dep, 64, 48, 128, o1=None) == B
    assert L.orbx_rgbd_depth(h, P(k), P(k), 1, C.c_void_p(depf.ctypes.data + 2), 1, 32, 48, 256, 1.0, 40.0, P(ur), P(dp)) == B  # misaligned
    assert one(0, dep, 64, 48, 128) == _capi.NO_DEVICE    # well-formed: reaches the device step
    assert one(1, depf, 64, 48, 256) == _capi.NO_DEVICE
    assert L.orbx_rgbd_depth(None, P(k), P(k), 1, P(dep), 0, 64, 48, 128, 1.0, 40.0, P(ur), P(dp)) == B
    # the device entry point
    cnt = np.zeros(2, np.int32); k4 = np.array(TUM_K, np.float32); d5 = np.array(TUM_D, np.float32)
    dev = lambda nf, cap, fmt, st, fs, dd=d5, nd=5, c=cnt: L.orbx_rgbd_depth_device(
        h, nf, P(k), P(c) if c is not None else None, cap, P(k4), P(dd) if dd is not None else None, nd, P(dep), fmt, 64, 48, st, fs,
        1.0, 40.0, None, P(ur), P(dp))
    assert dev(0, 4, 0, 128, 128 * 48) == B and dev(2, 0, 0, 128, 128 * 48) == B
    assert dev(2, 4, 0, 128, 128 * 47) == B               # frames overlap
    assert dev(2, 4, 0, 128, 128 * 48 + 1) == B           # frame stride not a multiple of 2
    assert dev(2, 4, 3, 128, 128 * 48) == B and dev(2, 4, 0, 100, 128 * 48) == B
    assert dev(2, 4, 0, 128, 128 * 48, c=None) == B and dev(2, 4, 0, 128, 128 * 48, dd=None) == B
    assert dev(2, 4, 0, 128, 128 * 48, nd=15) == B
    assert dev(2, 4, 0, 128, 128 * 48) == _capi.NO_DEVICE
    assert dev(1, 4, 0, 128, 0) == _capi.NO_DEVICE        # one frame: the frame stride is not read
    # the batch entry point
    imgs = np.zeros((2, 48, 64), np.uint8)
    kk = np.zeros((2, 8), _capi.KP_DTYPE); ds = np.zeros((2, 8, 32), np.uint8); cc = np.zeros(2, np.int32)
    fu = np.zeros((2, 8), np.float32)
    deps = np.zeros((2, 48, 64), np.uint16)
    bat = lambda fmt=0, st=128, fs=128 * 48, out=kk: L.orbx_extract_rgbd_batch(
        h, 2, P(imgs), 64, 48, 64, 64 * 48, P(deps), fmt, st, fs, 1.0, P(k4), P(d5), 5, 40.0, P(kk), P(out) if out is not None else None,
        P(ds), P(cc), P(fu), P(fu), 8)
    assert bat(fmt=5) == B and bat(st=64) == B and bat(fs=100) == B and bat(out=None) == B
    assert bat() == _capi.NO_DEVICE
    with pytest.raises(OrbxError) as e:
        Frame(k, np.zeros((1, 32), np.uint8), 64, 48).ComputeStereoFromRGBD(ex, dep, 40.0, 1.0)
    assert e.value.status == _capi.NO_DEVICE


def test_kernel_has_no_scratch_and_rounds_the_division(built_lib):
    from test_pipeline_room import _kernel_metadata
    from test_abi import _device_disassembly
    meta = _kernel_metadata(built_lib)
    hits = [v for k, v in meta.items() if "k_rgbd" in k]
    assert len(hits) == 1 and int(hits[0]["private_segment_fixed_size"]) == 0
    asm = _device_disassembly(built_lib)
    m = re.search(r"<_Z6k_rgbd[^>]*>:\n(.*?)s_endpgm", asm, re.S)
    assert m, "k_rgbd not in the code object"
    body = m.group(1)
    # mbf / d: the correctly rounded sequence (scale, reciprocal estimate, fused correction, fixup), not a bare reciprocal
    for op in ("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32"):
        assert op in body, op


def _build_harness(out):
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", "-shared", "-fPIC", "-I" + HERE,
           "-I" + os.path.join(ROOT, "tests", "compat_runtime"), "-I" + os.path.join(ROOT, "compat"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "harness.cpp"), "-L" + LIBDIR, "-lorbx",
           "-Wl,-rpath," + LIBDIR, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def test_compat_rgbd_body_compiles_without_warnings(built_lib, tmp_path):
    assert shutil.which("g++")
    p = _build_harness(str(tmp_path / "rgbd.so"))
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]


# ----------------------------------------------------------------------------------------------- GPU helpers
def rgb_frames(w, h, n, sid):
    g = synth.stream(w, h, n, stream_id=sid)
    return np.ascontiguousarray(np.stack([g, 255 - g, np.roll(g, 3, axis=2)], axis=-1))


def model_frame(kps, kun, depth, scale, mbf):
    return M.rgbd_depth(kps["x"], kps["y"], kun["x"], depth, scale, mbf)


def assert_frame(got, orc_k, orc_d, depth, K, D, scale, mbf, tag):
    k, ku, d, ur, dp = got
    assert len(k) == len(orc_k) and k.tobytes() == orc_k.tobytes() and d.tobytes() == orc_d.tobytes(), tag
    oku = oracle.undistort_keypoints(orc_k, K, D)
    assert ku.tobytes() == oku.tobytes(), tag
    mur, mdp = model_frame(orc_k, oku, depth, scale, mbf)
    assert np.array_equal(M.bits(ur), M.bits(mur)) and np.array_equal(M.bits(dp), M.bits(mdp)), tag


# ----------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,n,fmt,nfeat", [(640, 480, 64, "u16", 1000), (97, 131, 4, "u16", 300), (200, 96, 4, "f32", 200),
                                             (33, 41, 3, "u16", 50)])
def test_gpu_rgbd_batch_equals_oracle_and_model(w, h, n, fmt, nfeat):
    ex = ORBextractor(nfeat, 1.2, 8, 20, 7, max_batch=64, device=0)
    ex.set_input_format(_capi.FMT_RGB8)
    imgs = rgb_frames(w, h, n, 300 + w)
    deps = synth.depth_stream(w, h, n, stream_id=w, fmt=fmt)
    scale = depth_map_factor(5000.0) if fmt == "u16" else np.float32(1)
    res = ex.extract_rgbd_batch(imgs, deps, TUM_K, TUM_D, TUM_BF, scale)
    orc = oracle.OracleExtractor(nfeat, 1.2, 8, 20, 7)
    f7 = total = with_depth = 0
    for f in range(n):
        on, ok, od = orc.extract(oracle.cvt_gray(imgs[f]))
        assert on >= 0
        assert_frame(res[f], ok, od, deps[f], TUM_K, TUM_D, scale, TUM_BF, (w, h, f))
        total += on; f7 += M.f7_counts(ok["x"], ok["y"], w, h)[1]; with_depth += int((res[f][4] > 0).sum())
    assert total > 0 and f7 > 0      # F7 occurs at every one of these geometries
    assert with_depth > 0 or w < 64   # at 33 x 41 the +19 px offset sends most samples past the image


def _device_resident(ex, imgs_gray, deps, fmt, K, D, scale, mbf):
    import torch
    n, h, w = imgs_gray.shape
    cap = ex.max_keypoints(w, h)
    dev = torch.device("cuda:0")
    d_img = torch.from_numpy(imgs_gray).to(dev)
    d_dep = torch.from_numpy(deps.view(np.uint8).reshape(n, -1)).to(dev)
    d_k = torch.zeros((n, cap * 28), dtype=torch.uint8, device=dev)
    d_ku = torch.full((n, cap * 28), 0xAB, dtype=torch.uint8, device=dev)
    d_d = torch.zeros((n, cap * 32), dtype=torch.uint8, device=dev)
    d_c = torch.zeros(n, dtype=torch.int32, device=dev); d_s = torch.zeros(n, dtype=torch.int32, device=dev)
    d_ur = torch.full((n, cap), 7.0, dtype=torch.float32, device=dev); d_dp = torch.full((n, cap), 7.0, dtype=torch.float32, device=dev)
    ex.extract_batch_device(d_img, n, w, h, w, w * h, d_k, d_d, d_c, d_s, cap)
    ex.rgbd_depth_device(n, d_k, d_c, cap, K, D, d_dep, _capi.DEPTH_U16 if fmt == "u16" else _capi.DEPTH_F32, w, h,
                         deps.strides[1], deps.strides[0], scale, mbf, d_ku, d_ur, d_dp)
    ex.synchronize()
    cnt = d_c.cpu().numpy()
    k = d_k.cpu().numpy().view(_capi.KP_DTYPE); ku = d_ku.cpu().numpy().view(_capi.KP_DTYPE)
    dsc = d_d.cpu().numpy().reshape(n, cap, 32); ur = d_ur.cpu().numpy(); dp = d_dp.cpu().numpy()
    for f in range(n):   # rows beyond a frame's count are untouched
        assert (ku[f, cnt[f]:].view(np.uint8) == 0xAB).all() and (ur[f, cnt[f]:] == 7).all() and (dp[f, cnt[f]:] == 7).all()
    return [(k[f, :cnt[f]], ku[f, :cnt[f]], dsc[f, :cnt[f]], ur[f, :cnt[f]], dp[f, :cnt[f]]) for f in range(n)]


def _same(a, b, tag):
    assert len(a) == len(b), tag
    for f, (x, y) in enumerate(zip(a, b)):
        for i, (u, v) in enumerate(zip(x, y)):
            assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), (tag, f, i)


@pytest.mark.gpu
def test_gpu_paths_agree_chunked_pinned_and_both_modes(monkeypatch):
    w, h = 160, 120
    gray_all = synth.stream(w, h, 200, stream_id=71)
    dep_all = synth.depth_stream(w, h, 200, stream_id=71)
    scale = depth_map_factor(5000.0)
    ex = ORBextractor(300, 1.2, 8, 20, 7, max_batch=64, device=0)
    ref = _device_resident(ex, gray_all, dep_all, "u16", TUM_K, TUM_D, scale, TUM_BF)
    pin_dep = _capi.PinnedArray(dep_all.shape, np.uint16); pin_dep.array[:] = dep_all
    pin_img = _capi.PinnedArray(gray_all.shape, np.uint8); pin_img.array[:] = gray_all
    for n in (1, 63, 64, 65, 200):
        for mode in ("upload", "inplace"):
            monkeypatch.setenv("ORBX_RGBD_DEPTH", mode)
            _same(ex.extract_rgbd_batch(gray_all[:n], dep_all[:n], TUM_K, TUM_D, TUM_BF, scale), ref[:n], ("pageable", n, mode))
            _same(ex.extract_rgbd_batch(pin_img.array[:n], pin_dep.array[:n], TUM_K, TUM_D, TUM_BF, scale), ref[:n], ("pinned", n, mode))
    # page-locked outputs are written in place
    cap = ex.max_keypoints(w, h)
    outs = [_capi.PinnedArray((65, cap), _capi.KP_DTYPE), _capi.PinnedArray((65, cap), _capi.KP_DTYPE),
            _capi.PinnedArray((65, cap, 32), np.uint8), _capi.PinnedArray((65,), np.int32),
            _capi.PinnedArray((65, cap), np.float32), _capi.PinnedArray((65, cap), np.float32)]
    _same(ex.extract_rgbd_batch(pin_img.array[:65], pin_dep.array[:65], TUM_K, TUM_D, TUM_BF, scale,
                                out=tuple(o.array for o in outs)), ref[:65], "zero-copy outputs")
    # single-frame path (the compat body's entry point) on the batch's keypoints
    for f in (0, 64, 199):
        k, ku, _, ur, dp = ref[f]
        F = Frame(k, np.zeros((len(k), 32), np.uint8), w, h)
        F.mvKeysUn = ku
        sur, sdp = F.ComputeStereoFromRGBD(ex, dep_all[f], TUM_BF, scale)
        assert sur.tobytes() == ur.tobytes() and sdp.tobytes() == dp.tobytes(), f
    # no distortion: mvKeysUn is mvKeys
    r0 = ex.extract_rgbd_batch(gray_all[:3], dep_all[:3], TUM_K, (0.0, 0.0, 0.0, 0.0), TUM_BF, scale)
    for k, ku, _, _, _ in r0:
        assert k.tobytes() == ku.tobytes()


@pytest.mark.gpu
def test_gpu_f32_strided_depth_all_paths():
    w, h = 97, 131
    gray = synth.stream(w, h, 5, stream_id=13)
    dep = synth.depth_stream(w, h, 5, stream_id=13, fmt="f32")
    wide = np.full((5, h, w + 7), 2.5, np.float32)     # 7 gap floats per row, positive: a wrap into the gap reads them
    wide[:, :, :w] = dep
    view = wide[:, :, :w]
    ex = ORBextractor(300, 1.2, 8, 20, 7, max_batch=2, device=0)
    orc = oracle.OracleExtractor(300, 1.2, 8, 20, 7)
    for scale in (np.float32(1), np.float32(1 + 1e-6), np.float32(1.5), np.float32(2e-4)):
        res = ex.extract_rgbd_batch(gray, view, TUM_K, TUM_D, TUM_BF, scale)
        for f in range(5):
            on, ok, od = orc.extract(gray[f])
            assert_frame(res[f], ok, od, view[f], TUM_K, TUM_D, scale, TUM_BF, (float(scale), f))


@pytest.mark.gpu
def test_gpu_adversarial_values():
    ex = ORBextractor(1000, device=0)
    W, H = 8, 6
    vals = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-45, 1.2e-38, 65535.0, 1.0, 3.5, 1e30], np.float32)
    rng = np.random.default_rng(5)
    # every pixel, a wrap, the boundary, F7 and bad coordinates
    xs = [x + 0.5 for x in range(W + 3)] * H + [W - 1.0, float(W), 7.9999, -0.0, -1e-8, np.nan, np.inf, 2.2e9, 1e38]
    ys = [float(y) for y in range(H) for _ in range(W + 3)] + [H - 1.0, H - 1.0, H - 1.0001, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0]
    k = keys(xs, ys)
    ku = k.copy(); ku["x"] = k["x"] * np.float32(0.75) + np.float32(3)
    f32 = rng.choice(vals, size=(H, W)).astype(np.float32)
    u16 = rng.choice(np.array([0, 1, 2, 65535, 5000, 7], np.uint16), size=(H, W))
    for depth in (f32, u16):
        for scale in (1.0, 1 + 1e-6, 1.5, 2e-4, -1.0, 0.0):
            for mbf in (40.0, 0.0, -40.0, 1e-30):
                F = Frame(k, np.zeros((len(k), 32), np.uint8), W, H)
                F.mvKeysUn = ku
                ur, dp = F.ComputeStereoFromRGBD(ex, depth, mbf, scale)
                mur, mdp = M.rgbd_depth(k["x"], k["y"], ku["x"], depth, scale, mbf)
                assert np.array_equal(M.bits(ur), M.bits(mur)) and np.array_equal(M.bits(dp), M.bits(mdp)), \
                    (depth.dtype, scale, mbf, np.nonzero(M.bits(ur) != M.bits(mur))[0][:5], np.nonzero(M.bits(dp) != M.bits(mdp))[0][:5])
    # subnormal depth survives as itself (no flush), +inf gives uR = xU
    F = Frame(keys([0.5, 1.5], [0.0, 0.0]), np.zeros((2, 32), np.uint8), 2, 1)
    ur, dp = F.ComputeStereoFromRGBD(ex, np.array([[1e-45, np.inf]], np.float32), 40.0, 1.0)
    assert M.bits(dp)[0] == 1 and dp[1] == np.inf and ur[1] == np.float32(1.5) and ur[0] == -np.inf


@pytest.mark.gpu
def test_gpu_mono_outputs_unchanged_by_interleaved_rgbd_calls():
    w, h = 320, 240
    gray = synth.stream(w, h, 70, stream_id=5)
    dep = synth.depth_stream(w, h, 70, stream_id=5)
    ex = ORBextractor(500, 1.2, 8, 20, 7, max_batch=32, device=0)
    before = ex.extract_batch(gray)
    one = ex(gray[3])
    ex.extract_rgbd_batch(gray[:40], dep[:40], TUM_K, TUM_D, TUM_BF, depth_map_factor(5000.0))
    mid = ex.extract_batch(gray)
    ex.extract_rgbd_batch(gray, dep, TUM_K, TUM_D, TUM_BF, depth_map_factor(5000.0))
    after = ex.extract_batch(gray)
    one2 = ex(gray[3])
    for a, b, c in zip(before, mid, after):
        assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1].tobytes() == b[1].tobytes() == c[1].tobytes()
    assert one[0].tobytes() == one2[0].tobytes() and one[1].tobytes() == one2[1].tobytes()


@pytest.mark.gpu
def test_gpu_compat_body_equals_model(built_lib, tmp_path):
    out = str(tmp_path / "rgbd.so")
    p = _build_harness(out)
    assert p.returncode == 0, p.stderr[-4000:]
    L = C.CDLL(out)
    L.rgbd_error.restype = C.c_char_p
    L.rgbd_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    w, h = 160, 120
    gray = synth.stream(w, h, 2, stream_id=17)
    dep = synth.depth_stream(w, h, 2, stream_id=17, fmt="f32")
    ex = ORBextractor(300, device=0)
    for f in range(2):
        k, _ = ex(gray[f])
        ku = oracle.undistort_keypoints(k, TUM_K, TUM_D)
        for extra in (0, 5):      # continuous, and a column range of a wider matrix
            wide = np.full((h, w + extra), 9.0, np.float32); wide[:, :w] = dep[f]
            ur = np.zeros(len(k), np.float32); dp = np.zeros(len(k), np.float32)
            assert L.rgbd_compute(k.ctypes.data, ku.ctypes.data, len(k), wide.ctypes.data, w, h, w + extra, TUM_BF,
                                  ur.ctypes.data, dp.ctypes.data) == 0, L.rgbd_error()
            mur, mdp = M.rgbd_depth(k["x"], k["y"], ku["x"], wide[:, :w], 1.0, TUM_BF)
            assert np.array_equal(M.bits(ur), M.bits(mur)) and np.array_equal(M.bits(dp), M.bits(mdp)), (f, extra)
            assert (dp > 0).sum() > len(k) // 2
    assert L.rgbd_compute(None, None, 0, wide.ctypes.data, w, h, w, TUM_BF, None, None) == 0   # N == 0


@pytest.mark.gpu
def test_gpu_rgbd_soak_seeded():
    rng = np.random.default_rng(2026)
    ex = ORBextractor(400, 1.2, 8, 20, 7, max_batch=8, device=0)
    orc = oracle.OracleExtractor(400, 1.2, 8, 20, 7)
    for it in range(6):
        w, h = int(rng.integers(40, 260)), int(rng.integers(40, 200))
        n = int(rng.integers(1, 12))
        fmt = "u16" if it % 2 == 0 else "f32"
        gray = synth.stream(w, h, n, stream_id=1000 + it)
        dep = synth.depth_stream(w, h, n, stream_id=1000 + it, fmt=fmt)
        pad = int(rng.integers(0, 9))
        wide = np.zeros((n, h, w + pad), dep.dtype); wide[:, :, :w] = dep
        view = wide[:, :, :w]
        scale = np.float32(rng.choice([1.0, 1.5, 2e-4, 1 / 5000.0]))
        D = TUM_D if rng.uniform() < 0.5 else TUM_D[:4]
        mbf = np.float32(rng.uniform(-10, 80))
        res = ex.extract_rgbd_batch(gray, view, TUM_K, D, mbf, scale)
        for f in range(n):
            on, ok, od = orc.extract(gray[f])
            assert_frame(res[f], ok, od, view[f], TUM_K, D, scale, mbf, (it, w, h, f))
