"""CPU proof of the in-place level-0 loads (csrc/orbx_inplace.h): tests/san_level0.cpp replays, lane by lane and through the
helpers the kernels use, every load k_fast_rows, k_pyr_resize_rows_l1 and k_describe issue against the caller's image, on a
heap buffer of exactly (H - 1) * stride + W bytes, built with AddressSanitizer + UndefinedBehaviorSanitizer.  Host only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inplace_level0_loads_stay_inside_the_frame_and_cover_what_is_read(tmp_path):
    exe = str(tmp_path / "san_level0")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_level0.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_geometry.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-3000:]
    assert " 0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, out[-3000:]
    for geo in ("640x480 stride 640", "752x480 stride 752", "1241x376 stride 1244", "1920x1080 stride 1920", "639x479 stride 640",
                "97x75 stride 100"):
        assert geo + ": status 0" in p.stdout, geo
