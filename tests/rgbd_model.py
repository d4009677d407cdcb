"""Independent restatement of the RGB-D depth step (Frame::ComputeStereoFromRGBD, reference src/Frame.cc:1179-1226, after
Tracking::GrabImageRGBD's conversion, src/Tracking.cc:327-332) with the F7 rule of DESIGN.md section 2.

Everything is float32 IEEE arithmetic in numpy; results are compared as bit patterns, so NaN never compares unequal to itself.
The model works on the BYTES the reference reads: the float image Tracking made, `pitch` bytes per row, and the keypoint's
sample at byte o = v * pitch + 4 * u of it."""
import numpy as np

U16, F32 = 0, 1
_LIMIT = np.float32(2147483648.0)


def depth_map_factor(f):
    """src/Tracking.cc:201-211: |f| < 1e-5 -> 1, otherwise 1.0f / f (float)"""
    f = np.float32(f)
    if abs(float(f)) < 1e-5:
        return np.float32(1)
    with np.errstate(all="ignore"):
        return np.float32(1) / f


def converts_f32(scale):
    """src/Tracking.cc:327: fabs(mDepthMapFactor - 1.0f) > 1e-5 (float difference, compared in double)"""
    with np.errstate(all="ignore"):
        return float(abs(np.float32(scale) - np.float32(1))) > 1e-5


def raw_bytes(depth):
    """the bytes of a (possibly row-strided) H x W depth view the reference may touch: (H - 1) full rows and the W samples of
    the last one, gaps between rows included"""
    d = np.asarray(depth)
    H, W = d.shape
    span = (H - 1) * d.strides[0] + W * d.itemsize
    rows = d.view(np.uint8)            # H x (W * itemsize) bytes, rows d.strides[0] apart
    return np.lib.stride_tricks.as_strided(rows, shape=(span,), strides=(1,)).copy()


def float_image(depth, scale):
    """(float image as float32 array over its bytes, pitch in bytes, limit = (H - 1) * pitch + 4 * W) as the reference reads it"""
    d = np.asarray(depth)
    H, W = d.shape
    scale = np.float32(scale)
    if d.dtype == np.uint16:   # convertTo(CV_32F, scale): a new continuous image, (float)raw * scale + 0.0f
        with np.errstate(all="ignore"):
            img = (np.ascontiguousarray(d).astype(np.float32) * scale + np.float32(0)).reshape(-1)
        return img, 4 * W, 4 * W * H
    assert d.dtype == np.float32 and d.strides[1] == 4
    pitch = d.strides[0]
    if pitch == 4 * W and not converts_f32(scale):   # continuous and read as it is: a view, no copy
        return d.reshape(-1), pitch, (H - 1) * pitch + 4 * W
    raw = raw_bytes(d)
    raw = np.concatenate([raw, np.zeros((-len(raw)) % 4, np.uint8)]).view(np.float32).copy()
    if converts_f32(scale):     # in place: only the W floats of every row, the gap keeps its bytes
        col = (np.arange(len(raw)) * 4) % pitch
        m = col < 4 * W
        with np.errstate(all="ignore"):
            raw[m] = raw[m] * scale + np.float32(0)
    return raw, pitch, (H - 1) * pitch + 4 * W


def sample_offset(x, y, pitch, limit):
    """byte offset of the sample of a keypoint at (x, y), or None under F7 (and for negative / non-finite / huge coordinates)"""
    x, y = np.float32(x), np.float32(y)
    if not (x >= 0 and y >= 0 and x < _LIMIT and y < _LIMIT):
        return None
    o = int(y) * pitch + 4 * int(x)      # int() truncates towards zero, as (int) does
    return None if o + 4 > limit else o


def rgbd_depth(kps_x, kps_y, kun_x, depth, scale, mbf):
    """(u_right, depth) float32 arrays for keypoints at (kps_x, kps_y) (mvKeys) with undistorted x kun_x (mvKeysUn)"""
    img, pitch, limit = float_image(depth, scale)
    n = len(kps_x)
    ur = np.full(n, -1, np.float32)
    dp = np.full(n, -1, np.float32)
    mbf = np.float32(mbf)
    for i in range(n):
        o = sample_offset(kps_x[i], kps_y[i], pitch, limit)
        if o is None:
            continue
        d = img[o // 4]
        if d > 0:
            dp[i] = d
            with np.errstate(all="ignore"):
                ur[i] = np.float32(kun_x[i]) - mbf / d
    return ur, dp


def f7_counts(kps_x, kps_y, W, H, pitch=None):
    """(row wraps inside the image's memory, samples past it) for a W x H image: u >= W with the sample inside, F7 cases"""
    pitch = 4 * W if pitch is None else pitch
    limit = (H - 1) * pitch + 4 * W
    wrap = past = 0
    for x, y in zip(kps_x, kps_y):
        o = sample_offset(x, y, pitch, limit)
        if o is None:
            past += 1
        elif o % pitch >= 4 * W or int(np.float32(x)) >= W:
            wrap += 1
    return wrap, past


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def rgbd_depth_vectorized(kps_x, kps_y, kun_x, depth, scale, mbf):
    """rgbd_depth without the Python loop (same float32 operations; tools/policy_rates.py times it as the CPU side)"""
    img, pitch, limit = float_image(depth, scale)
    x = np.asarray(kps_x, np.float32); y = np.asarray(kps_y, np.float32)
    with np.errstate(all="ignore"):
        ok = (x >= 0) & (y >= 0) & (x < _LIMIT) & (y < _LIMIT)
        o = np.where(ok, y, 0).astype(np.int64) * pitch + 4 * np.where(ok, x, 0).astype(np.int64)
        ok &= o + 4 <= limit
        d = np.where(ok, img[np.where(ok, o // 4, 0)], np.float32(-1))
        good = d > 0
        ur = np.where(good, np.asarray(kun_x, np.float32) - np.float32(mbf) / np.where(good, d, np.float32(1)), np.float32(-1))
        return ur.astype(np.float32), np.where(good, d, np.float32(-1)).astype(np.float32)
