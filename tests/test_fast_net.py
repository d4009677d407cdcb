"""CPU check of orbx_fast_net (csrc/orbx_fast_net.h), the corner test and score network both instances of fr_round (k_fast_rows) run:
tests/fast_net.cpp compares it with the definition written out directly -- the maximum over the 16 arcs of the minimum over 9 of
+-(ring - v) -- on planted arcs (every start, both polarities, margins th - 1 / th / th + 1 for th in 0, 1, 7, 20, 254, 255), on all
0 / 255 rings, on mb == md ties and on two million random rings, and checks the selection rule (larger compass margin first, the
other polarity when both pre-tests pass).  Built with AddressSanitizer + UndefinedBehaviorSanitizer.  Host only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_network_equals_the_definition_of_fast_9_16(tmp_path):
    exe = str(tmp_path / "fast_net")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "fast_net.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-3000:]
    m = re.search(r"^(\d+) cases, 0 failures$", p.stdout, re.M)
    assert m and int(m.group(1)) > 6_000_000, out[-3000:]
    assert "FAIL" not in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, out[-3000:]
