"""Writes the records of the compiled reference extractor (oracle/_ref/libref_extractor_{strict,fma}.so) that
tests/test_ref_extractor.py and the GPU tests of tests/test_gpu_parity.py compare with:

    tests/golden/ref_extractor_inputs_*.npz        every input image that is not already a fixture
    tests/golden/ref_extractor_{strict,fma}.json   per case: counts and sha256 per stage (pyramid, FAST candidates, keypoints
                                                   per level with angle bits, final keypoints, descriptors); the full keypoints
                                                   and descriptors where there are few; the rows in which the variants differ
    tests/golden/ref_extractor_contraction.json    (angle bits, tap) pairs at which GCC_FMA and STRICT give other coordinates

    python tools/ref_extractor_record.py --record      needs the reference tree (or a built oracle/_ref/); a test run never writes
    python tools/ref_extractor_record.py               compares what it would write with what is committed"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ref_extractor as X  # noqa: E402
from oracle import orb_oracle as oo  # noqa: E402

N_PAIRS = 96


def input_files():
    groups = {}
    for name, img in X.make_inputs().items():
        g, k = name.split("/")
        groups.setdefault(g, {})[k] = img
    return {"ref_extractor_inputs_%s.npz" % g: v for g, v in groups.items()}


def case_records():
    out = {v: {} for v in X.VARIANTS}
    stages = {}
    for name, inp, p, _ in X.CASES + X.MODE_CASES:
        for v in X.VARIANTS:
            st = stages[name, v] = X.cpu_stages(X.RefExtractor(v, *p), X.inputs()[inp], p[2])
            rec = X.digest(st)
            rec["input"], rec["params"] = inp, list(p)
            if 0 <= st["n"] <= X.FULL_OUTPUT_MAX or (st["n"] > 0 and X.inputs()[inp].size <= X.FULL_OUTPUT_AREA):
                rec["full_kps"] = st["kps"].ravel().tolist()
                rec["full_desc"] = st["desc"].ravel().tolist()
            out[v][name] = rec
        a, b = stages[name, "strict"], stages[name, "fma"]
        if a["n"] == b["n"] and a["n"] > 0:
            rows = np.nonzero((a["desc"] != b["desc"]).any(axis=1) | (a["kps"] != b["kps"]).any(axis=1))[0]
            for v, st in (("strict", a), ("fma", b)):
                out[v][name]["rows_differing_between_variants"] = {
                    str(int(r)): {"kps": st["kps"][r].tolist(), "desc": st["desc"][r].tolist()} for r in rows}
    for v in X.VARIANTS:       # after contraction.json is written: the direct entries on the seeded inputs of tests/ref_extractor.py
        out[v]["_direct"] = {k: {"n": int(a.size), "sha256": X.sha(a)} for k, a in X.direct_results("ref", v).items()}
    return out


def contraction_pairs():
    """random float32 angles in [0, 360); a pair is kept when its coordinates differ between the modes AND the two oracle modes
    differ in that tap's descriptor bit on at least one of the seeded images (then the test can tell which product is fused)"""
    rng = np.random.default_rng(4)
    px, py = X.pattern_xy()
    images = [X.contraction_image(s) for s in X.CONTRACTION_SEEDS]
    pairs = []
    while len(pairs) < N_PAIRS:
        ang = rng.uniform(0, 360, 4000).astype(np.float32)
        a, b = X.cosf_sinf(ang)
        (ixs, iys), (ixf, iyf) = X.tap_coordinates(a, b, px, py)
        for i, t in zip(*np.nonzero((ixs != ixf) | (iys != iyf))):
            byte, bit = t // 16, (t // 2) % 8
            for im in images:
                d0 = X.oracle_descriptor(im, 32, 32, ang[i], oo.FP_GCC_FMA)
                d1 = X.oracle_descriptor(im, 32, 32, ang[i], oo.FP_STRICT)
                if (d0[byte] ^ d1[byte]) >> bit & 1:
                    pairs.append([int(ang[i:i + 1].view(np.uint32)[0]), int(t)])
                    break
    return {"what": "[float32 bits of kpt.angle in degrees, tap index 0..511 into the pattern]", "pairs": pairs[:N_PAIRS]}


def main():
    record = "--record" in sys.argv
    if not X.reference_available():
        sys.exit("neither the reference tree nor oracle/_ref/libref_extractor_*.so is here")
    bad = 0
    for f, arrays in input_files().items():
        path = os.path.join(X.GOLD, f)
        if record:
            np.savez_compressed(path, **arrays)
            print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
        else:
            with np.load(path) as z:
                same = sorted(z.files) == sorted(arrays) and all(np.array_equal(z[k], arrays[k]) for k in arrays)
            print("%s: %s" % (f, "same" if same else "DIFFERENT"))
            bad += not same
    X._INPUTS = None
    todo = [("ref_extractor_contraction.json", contraction_pairs)] + [("ref_extractor_%s.json" % v, (lambda v=v: records()[v])) for v in X.VARIANTS]
    made = {}

    def records():
        if not made:
            made.update(case_records())
        return made
    for f, make in todo:
        obj = make()
        path = os.path.join(X.GOLD, f)
        if record:
            with open(path, "w") as fh:
                json.dump(obj, fh, separators=(",", ":"), sort_keys=True)
                fh.write("\n")
            print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
        else:
            with open(path) as fh:
                same = json.load(fh) == json.loads(json.dumps(obj))
            print("%s: %s" % (f, "same" if same else "DIFFERENT"))
            bad += not same
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
