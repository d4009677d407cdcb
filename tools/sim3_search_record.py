"""Records what the reference's compiled src/ORBmatcher.cc (oracle/_ref/libref_matcher_{strict,fma}.so) returns for every problem
of every scene of tests/sim3_search_scenes.py: tests/golden/sim3_search_{strict,fma}.json, small integers only (counts, and the
match vectors in the entry() convention of tests/test_ref_matcher.py).  Without --record it compares and reports; a test run
never writes the records."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import sim3_search_scenes as sc  # noqa: E402
from orb_slam2_detailed_comments_amd import ORBextractor, _capi  # noqa: E402
from test_ref_matcher import entry, ref_harness, reference_available  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "sim3_search_%s.json")


def main():
    assert reference_available(), "needs the reference tree or oracle/_ref/"
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    thr = np.zeros(16, np.float32)
    _capi.check(_capi.lib().orbx_predict_scale_table(ex.handle, _capi.ptr(thr), 16))
    scenes = sc.all_scenes(thr)
    bad = 0
    for variant in ("strict", "fma"):
        H = ref_harness(variant)
        rec = {}
        for name, s in scenes.items():
            for k, (n, m) in enumerate(sc.harness_search(H, s)):
                rec["%s/%d" % (name, k)] = dict(n=n, matches=entry(m))
        path = GOLDEN % variant
        if "--record" in sys.argv:
            with open(path, "w") as f:
                json.dump(rec, f, indent=0, sort_keys=True)
                f.write("\n")
            print("wrote", path, len(rec), "problems,", sum(r["n"] for r in rec.values()), "matches")
        else:
            with open(path) as f:
                same = json.load(f) == rec
            bad += not same
            print(path, "unchanged" if same else "DIFFERS")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
