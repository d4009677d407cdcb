"""compat/ORBextractor.h built with -DORBX_COMPAT_PYRAMID_MODE=ORBX_PYRAMID_UPSTREAM, executed against the cv::Mat stand-in of
tests/compat_runtime/: operator() gives the upstream model's keypoints and descriptors, and the public mvImagePyramid holds
the un-padded levels."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import upstream_model as um
from compat_scenes import F32, KP, Harness, Scene, i32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNTIME = os.path.join(ROOT, "tests", "compat_runtime")
LIBDIR = os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "lib")


def _build(out):
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", "-shared", "-fPIC", "-DORBX_COMPAT_PYRAMID_MODE=ORBX_PYRAMID_UPSTREAM",
           "-I" + RUNTIME, "-I" + os.path.join(ROOT, "compat"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(RUNTIME, "harness.cpp"), os.path.join(RUNTIME, "map_model.cpp"), "-L" + LIBDIR, "-lorbx",
           "-Wl,-rpath," + LIBDIR, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def H(built_lib, tmp_path_factory):
    assert shutil.which("g++")
    out = str(tmp_path_factory.mktemp("compat_upstream") / "harness.so")
    p = _build(out)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]
    return Harness(out)


def test_harness_builds_in_upstream_mode(H):
    assert H is not None


@pytest.mark.gpu
def test_shim_extracts_the_upstream_model_and_holds_unpadded_levels(H):
    S = Scene(H)   # noqa: F841  (keeps the harness' objects alive for the test, as in tests/test_compat_runtime.py)
    img = um.block_image(3, 300, 200, 6)
    M = um.ModelExtractor(1000, 1.2, 8, 20, 7, padded=False)
    mn, mk, md = M.extract(img)
    ex, n = i32(), i32()
    H("h_extractor_new", 1000, F32(1.2), 8, 20, 7, ex)
    cap = 1000 + 64 * 8
    k, d = np.zeros(cap, KP), np.zeros((cap, 32), np.uint8)
    H("h_extract", int(ex[0]), img, 300, 200, k, d, cap, n)
    assert n[0] == mn > 600
    assert k[:mn].tobytes() == mk.tobytes() and d[:mn].tobytes() == md.tobytes()
    pw, ph = i32(), i32()
    for l in range(8):
        H("h_pyramid", int(ex[0]), l, None, 0, pw, ph)
        want = M.level_image(l)
        assert (ph[0], pw[0]) == want.shape
        buf = np.zeros(pw[0] * ph[0], np.uint8)
        H("h_pyramid", int(ex[0]), l, buf, len(buf), pw, ph)
        assert np.array_equal(buf.reshape(ph[0], pw[0]), want), l
