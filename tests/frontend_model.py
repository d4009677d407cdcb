"""Independent models of the kernels that turn a camera frame into level 0 and mvKeysUn: cv::remap (k_pyr_l0_remap and the
host digest of orbx_set_rectification), cv::cvtColor to gray (k_pyr_l0_color), cvUndistortPoints with R = I, P = K (k_undistort,
k_rgbd) and the reflect-101 frame of level 0.  Plain numpy, written from the rules below, not from the C code; never calls the
oracle or the library.

remap rule (OpenCV 3.2, INTER_LINEAR, CV_32FC1 maps, BORDER_CONSTANT 0):
    p = float32(map) * float32(32)
    s = rint(p), half to even; where p is NaN or not in [-2^31, 2^31): s = INT_MIN (the x86 "integer indefinite")
    i = clip(s >> 5, -32768, 32767) (arithmetic shift), f = s & 31
    taps (ix + k2, iy + k1), k1, k2 in {0, 1}; a tap outside the image reads 0
    result = floor(exact + 1/2), exact = sum of taps times (32 - fx | fx)(32 - fy | fy) / 1024
The four weights times 32 are the integers of OpenCV's table and sum to 2^15, so floor(exact + 1/2) = (acc + 2^14) >> 15 with no
tolerance; remap() computes both forms in integers and asserts that they agree."""
import numpy as np

INT_MIN = -(1 << 31)
EDGE = 19   # EDGE_THRESHOLD: the reflect-101 frame of every pyramid level


def digest_full(mx, my):
    """per map entry: dict of int64 arrays sx, sy (the 32-bit cvRound), ix, iy, fx, fy and bool arrays bad_x, bad_y (the conversion
    gave INT_MIN, the integer indefinite)"""
    out = {}
    for name, m in (("x", mx), ("y", my)):
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.asarray(m, np.float32) * np.float32(32)
            assert p.dtype == np.float32
            ok = (p >= np.float32(-2147483648.0)) & (p < np.float32(2147483648.0))     # False for NaN
            r = np.rint(np.where(ok, p, np.float32(0)))                                   # half to even, float32
        s = np.where(ok, r.astype(np.float64).astype(np.int64), INT_MIN)
        out["s" + name] = s
        out["bad_" + name] = s == INT_MIN       # (-2^26 * 32 = -2^31 converts to the same word without being out of range)
        out["i" + name] = np.clip(s >> 5, -32768, 32767)
        out["f" + name] = s & 31
    return out


def digest(mx, my):
    d = digest_full(mx, my)
    return d["ix"], d["iy"], d["fx"], d["fy"]


def packed_digest(mx, my):
    """(xy, frac) as orbx_debug_rect_digest writes them: ix | iy << 16 (int16 each), fy << 5 | fx"""
    ix, iy, fx, fy = digest(mx, my)
    xy = (ix & 0xffff) | ((iy & 0xffff) << 16)
    return xy.astype(np.uint32), ((fy << 5) | fx).astype(np.uint32)


def remap(img, mx, my):
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    ix, iy, fx, fy = digest(mx, my)
    acc = np.zeros(ix.shape, np.int64)
    for k1 in (0, 1):
        for k2 in (0, 1):
            xx, yy = ix + k2, iy + k1
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            tap = np.where(inside, img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64), 0)
            acc += (fx if k2 else 32 - fx) * (fy if k1 else 32 - fy) * tap
    out = (acc + 512) >> 10                                    # floor(acc / 1024 + 1/2)
    assert np.array_equal(out, (acc * 32 + (1 << 14)) >> 15)   # OpenCV's form: weights * 32 sum to 2^15
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def zero_fraction_entry_is_the_plain_weight():
    """OpenCV's table entry at fx = fy = 0 is {32767, 0, 0, 1}, not {32768, 0, 0, 0}: the same byte for every (p00, p11)"""
    p00, p11 = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    return np.array_equal((32767 * p00 + p11 + (1 << 14)) >> 15, p00)


def cvt_gray(img, r_off, b_off):
    """img [..., H, W, C] uint8, C = 3 or 4: (R*4899 + G*9617 + B*1868 + 8192) >> 14; a fourth channel is not read"""
    a = np.asarray(img, np.uint8).astype(np.int64)
    g = (a[..., r_off] * 4899 + a[..., 1] * 9617 + a[..., b_off] * 1868 + 8192) >> 14
    assert g.max() <= 255
    return g.astype(np.uint8)


def pad101(img, border=EDGE):
    """the padded level: `border` pixels of reflect-101 (dcb|abcd|cba) on every side"""
    return np.pad(np.asarray(img), border, mode="reflect")


def undistort(x, y, K, dist):
    """cvUndistortPoints, R = I, P = K: float32 points and parameters converted to float64, five fixed iterations, operation
    order as stated in oracle/orb_oracle_match.c:925-947, float32 results.  dist: up to 14 float32 coefficients, of which
    k[0..11] are evaluated.  No identity rule here (undistort_keypoints has it)."""
    k = np.zeros(14, np.float64)
    d = np.asarray(dist, np.float32)
    k[:len(d)] = d.astype(np.float64)
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in K)
    ifx, ify = np.float64(1.0) / fx, np.float64(1.0) / fy
    x = np.asarray(x, np.float32).astype(np.float64); y = np.asarray(y, np.float32).astype(np.float64)
    x0 = x = (x - cx) * ifx
    y0 = y = (y - cy) * ify
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    xx = fx * x + 0.0 * y + cx
    yy = 0.0 * x + fy * y + cy
    ww = 1.0 / (0.0 * x + 0.0 * y + 1.0)
    return (xx * ww).astype(np.float32), (yy * ww).astype(np.float32)


def undistort_keypoints(kps, K, dist):
    """mvKeysUn from mvKeys: a copy when there is no coefficient or dist[0] == 0 (src/Frame.cc:772-776)"""
    out = kps.copy()
    d = np.asarray(dist, np.float32)
    if len(d) < 1 or d[0] == 0.0:
        return out
    out["x"], out["y"] = undistort(kps["x"], kps["y"], K, d)
    return out


def image_bounds(cols, rows, K, dist):
    """Frame::ComputeImageBounds: mnMinX, mnMaxX, mnMinY, mnMaxY (float32)"""
    d = np.asarray(dist, np.float32)
    if len(d) < 1 or d[0] == 0.0:
        return np.array([0, cols, 0, rows], np.float32)
    x, y = undistort(np.array([0, cols, 0, cols], np.float32), np.array([0, 0, rows, rows], np.float32), K, d)
    return np.array([min(x[0], x[2]), max(x[1], x[3]), min(y[0], y[1]), max(y[2], y[3])], np.float32)
