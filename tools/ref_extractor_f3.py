"""The F3 measurement: how often does the reference's sort tie-break by node ADDRESS change the output when the
std::list nodes come from glibc malloc (libref_extractor_strict_plain.so) instead of an allocator whose addresses follow
allocation order (libref_extractor_strict.so)?  Runs both over the cases of tests/ref_extractor.py and 200 synthetic frames of
160 x 120 and prints the share of frames that differ, and whether they differ in list order only or in the selected set.
A measurement, not a test: the answer depends on the allocator and on the heap's history."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ref_extractor as X  # noqa: E402
from orb_slam2_detailed_comments_amd import synth  # noqa: E402


def compare(img, p):
    a = X.cpu_stages(X.RefExtractor("strict", *p), img, p[2])
    b = X.cpu_stages(X.RefExtractor("strict_plain", *p), img, p[2])
    if a["n"] == b["n"] and np.array_equal(a["kps"], b["kps"]) and np.array_equal(a["desc"], b["desc"]):
        return "same"
    rows = lambda st: sorted(bytes(k) + bytes(d) for k, d in zip(st["kps"], st["desc"]))
    return "order" if rows(a) == rows(b) else "set"


def main():
    assert X.reference_available()
    frames = [(c[0], X.inputs()[c[1]], c[2]) for c in X.CASES + X.MODE_CASES]
    for sid in range(20):
        sc = synth.Scene(160, 120, 500 + sid)
        frames += [("synth%d_%d" % (sid, t), sc.frame(t), (1000, 1.2, 8, 20, 7)) for t in range(10)]
    tally = {"same": 0, "order": 0, "set": 0}
    for name, img, p in frames:
        r = compare(img, p)
        tally[r] += 1
        if r != "same":
            print("%-24s differs in the %s" % (name, "list order only" if r == "order" else "selected set"))
    n = len(frames)
    print("%d frames: %d identical, %d differ in list order only, %d differ in the selected set (%.1f %% differ)"
          % (n, tally["same"], tally["order"], tally["set"], 100.0 * (n - tally["same"]) / n))


if __name__ == "__main__":
    main()
