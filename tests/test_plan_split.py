"""CPU check of orbx_split_batch (csrc/orbx_internal.h), the sub-batch offsets both multi-stream launch plans of run_chunk use:
tests/plan_split.cpp walks B = 8..1100, S = 1..8 and both head modes, built with AddressSanitizer + UndefinedBehaviorSanitizer.
Host only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_offsets_cover_the_batch_in_multiples_of_eight(tmp_path):
    exe = str(tmp_path / "plan_split")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "plan_split.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-3000:]
    assert "17488 cases, 0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, out[-3000:]
