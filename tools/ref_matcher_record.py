"""Writes tests/golden/ref_matcher_{strict,fma}.json: the outputs of the compiled reference matcher (oracle/_ref/
libref_matcher_*.so, built from the reference tree by oracle/ref/build_ref.py) for every case of tests/test_ref_matcher.py.

    python tools/ref_matcher_record.py            compares a fresh run with the files and says what differs
    python tools/ref_matcher_record.py --record   rewrites the files

A test run never writes them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_ref_matcher as T  # noqa: E402


def main():
    if not T.reference_available():
        sys.exit("no compiled reference and no reference tree to build it from (%s)" % T.B.reference_dir())
    status = 0
    for variant in T.VARIANTS:
        out = T.reference_outputs(variant)
        path = T.GOLDEN % variant
        if "--record" in sys.argv:
            with open(path, "w") as f:
                json.dump(out, f, sort_keys=True, separators=(",", ":"))
                f.write("\n")
            print("%s: %d cases, %d bytes" % (path, len(out), os.path.getsize(path)))
        else:
            old = json.load(open(path)) if os.path.exists(path) else {}
            diff = sorted(c for c in set(old) | set(out) if old.get(c) != out.get(c))
            print("%s: %s" % (path, "reproduced" if not diff else "differs in %s" % diff))
            status |= bool(diff)
    sys.exit(status)


if __name__ == "__main__":
    main()
