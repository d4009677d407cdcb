"""compat/Initializer_ransac.inl (the replacement for the two threads of Initializer::Initialize, src/Initializer.cc:204-215)
compiled against the stand-ins of tests/compat_init/ and the cv::Mat of tests/compat_runtime/, linked against liborbx.so and run:
mvMatches12 made from a vMatches12 with unmatched keypoints, the marshalling of mvKeys1 / mvKeys2 (ALL keypoints) and mvSets,
vbMatchesInliersH / F, SH, SF, H, F and the RH the next line of Initialize computes -- against tests/init_model.py for the same
draws, bit for bit; a scene where nothing scores leaves both matrices empty.  On a host-only handle here (through the
fragment's ORBX_INITIALIZER_HANDLE hook); under the gpu marker on the device, on the thread_local handle the fragment creates."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import init_model as im
import init_scenes as sc
from orb_slam2_detailed_comments_amd import ORBextractor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "lib")
F = np.float32


def build(tmp, shared):
    assert shutil.which("g++")
    out = str(tmp / ("harness_shared.so" if shared else "harness_own.so"))
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "tests", "compat_init"),
           "-I" + os.path.join(ROOT, "tests", "compat_runtime"), "-I" + os.path.join(ROOT, "compat"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "compat_init", "harness.cpp"), "-L" + LIBDIR, "-lorbx", "-Wl,-rpath," + LIBDIR, "-o", out]
    if shared:
        cmd.insert(1, "-DCI_SHARED_HANDLE")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]
    L = C.CDLL(out)
    L.ci_error.restype = C.c_char_p
    L.ci_run.restype = C.c_int
    vp, i32 = C.c_void_p, C.c_int
    L.ci_run.argtypes = [vp, i32, vp, i32, vp, vp, C.c_float, i32, vp] + [vp] * 8 + [i32, vp]
    return L


def sorted_by_frame1(p):
    """Initialize builds mvMatches12 by walking frame 1's keypoints in order, so the matches of a scene are taken in that order
    and the draws, which index mvMatches12, stay as they are: it is the same problem with its matches renumbered"""
    order = np.argsort(p["matches"][:, 0], kind="stable")
    return sc.variant(p, matches=p["matches"][order], planted_inlier=p["planted_inlier"][order])


def check(L, handle, p):
    p = sorted_by_frame1(p)
    k1, k2, m = np.ascontiguousarray(p["keys1"], F), np.ascontiguousarray(p["keys2"], F), p["matches"]
    vm = np.full(len(k1), -1, np.int32)
    vm[m[:, 0]] = m[:, 1]
    n = len(m)
    sets = np.ascontiguousarray(p["sets"], np.int32)
    s = np.zeros(3, F)
    H9, F9, has = np.zeros(9, F), np.zeros(9, F), np.full(2, -9, np.int32)
    iH, iF, mo_out = np.full(n + 1, 9, np.uint8), np.full(n + 1, 9, np.uint8), np.full((n + 1, 2), -9, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)                 # noqa: E731
    rc = L.ci_run(handle, len(k1), P(k1), len(k2), P(k2), P(vm), float(p["sigma"]), int(p["iterations"]), P(sets), s[0:].ctypes.data,
                  s[1:].ctypes.data, s[2:].ctypes.data, P(H9), P(F9), P(has), P(iH), P(iF), n, P(mo_out))
    assert rc == n, L.ci_error().decode()
    assert np.array_equal(mo_out[:n], m) and iH[n] == 9 and iF[n] == 9
    mo = im.solve(p)
    assert sc.bits(s[0]) == sc.bits(mo["SH"]) and sc.bits(s[1]) == sc.bits(mo["SF"])
    with np.errstate(all="ignore"):
        assert sc.bits(s[2]) & 0x7fffffff == sc.bits(mo["SH"] / (mo["SH"] + mo["SF"])) & 0x7fffffff      # RH as Initialize computes it
    for name, model, M9, mask, got in (("H", im.H, H9, iH, has[0]), ("F", im.FUND, F9, iF, has[1])):
        it = mo["it" + name]
        assert got == (it >= 0), name                          # no iteration scored: the cv::Mat stays empty
        if it >= 0:
            assert np.array_equal(sc.bits(M9), sc.bits(mo["per"][model]["M"][it].reshape(-1))), name
            assert np.array_equal(mask[:n].astype(bool), mo["per"][model]["masks"][it]), name
        else:
            assert not mask[:n].any(), name
    return mo, p, (iH[:n].astype(bool), iF[:n].astype(bool))


def all_scenes(L, handle):
    for k, p in enumerate(sc.planted_scenes()):
        mo, q, (iH, iF) = check(L, handle, p)
        want = im.FUND if p["kind"] == "general" else im.H
        assert mo["model"] == want and ((iH if want == im.H else iF) == q["planted_inlier"]).all(), k
    check(L, handle, sc.degenerate())
    a, b, _ = sc.none_scenes()
    for p in (a, b):
        mo, _, _ = check(L, handle, p)
        assert mo["model"] == im.NONE


def test_fragment_equals_the_model_on_a_host_only_handle(built_lib, tmp_path):
    L = build(tmp_path, shared=True)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    try:
        all_scenes(L, ex.handle)
    finally:
        ex.close()


@pytest.mark.gpu
def test_fragment_equals_the_model_on_its_own_device_handle(built_lib, tmp_path):
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=True)
    try:
        all_scenes(build(tmp_path, shared=False), None)
    finally:
        faulthandler.cancel_dump_traceback_later()
