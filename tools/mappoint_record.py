"""Writes tests/golden/mappoint_batch_{strict,fma}.json from the reference's compiled src/MapPoint.cc (oracle/_ref/, built from
the reference tree when it is there): the seeded scene of tests/test_mappoint_batch_cpu.py played into the compiled harness,
ComputeDistinctiveDescriptors called on every point, and the descriptors it leaves hashed.  best_idx / best_median are those of
tests/mappoint_model.py, recorded only after the model's descriptor equalled the reference's on every point (the harness
exports the descriptor alone).  A test run never writes these files.

    python tools/mappoint_record.py --record
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import mappoint_model as mm  # noqa: E402
import test_mappoint_batch_cpu as T  # noqa: E402
from test_ref_matcher import VARIANTS, ref_harness, reference_available  # noqa: E402


def main():
    if "--record" not in sys.argv:
        sys.exit(__doc__)
    if not reference_available():
        sys.exit("neither oracle/_ref/libref_matcher_*.so nor the reference tree is here")
    ob, desc, idx, med, best = T.golden_scene()
    for variant in VARIANTS:
        out, rows = T.play_reference(ref_harness(variant), ob, desc)
        for p in range(len(ob) - 1):
            assert np.array_equal(out[p], best[p]), ("the model differs from the compiled reference", variant, p)
        with open(T.GOLDEN % variant, "w") as f:
            json.dump(T.record(idx, med, out), f)
            f.write("\n")
        print(T.GOLDEN % variant, mm.desc_hash(out))


if __name__ == "__main__":
    main()
