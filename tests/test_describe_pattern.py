"""The two per-lane forms of the BRIEF pattern k_describe can read (c_pattern_lane, int8; c_pattern_f32, float): the float table
is the int8 one element for element, and both are the shared header's 256 pairs dealt over 64 lanes x 4 rounds.  Host only."""
import numpy as np
from orb_slam2_detailed_comments_amd import _capi
from ref_extractor import pattern_xy


def _tables():
    i8 = np.zeros(1024, np.int8); f32 = np.full(1024, np.nan, np.float32)
    _capi.check(_capi.lib().orbx_debug_describe_pattern(_capi.ptr(i8), _capi.ptr(f32)))
    return i8, f32


def test_float_pattern_equals_int8_pattern():
    i8, f32 = _tables()
    assert f32.dtype == np.float32 and np.isfinite(f32).all()
    assert np.array_equal(f32, i8.astype(np.float32))          # element for element
    assert np.array_equal(f32.astype(np.int64), i8.astype(np.int64))
    assert f32.view(np.uint32).tolist() == i8.astype(np.float32).view(np.uint32).tolist()   # bit for bit (no -0.0)


def test_lane_layout_is_the_headers_pattern():
    i8, _ = _tables()
    px, py = pattern_xy()                                       # 512 points: pair p = points 2p, 2p + 1
    lane = i8.reshape(64, 4, 4)                                 # [lane][round] = x1, y1, x2, y2 of pair round * 64 + lane
    for r in range(4):
        p = r * 64 + np.arange(64)
        want = np.stack([px[2 * p], py[2 * p], px[2 * p + 1], py[2 * p + 1]], axis=1)
        assert np.array_equal(lane[:, r, :].astype(np.int64), want)
