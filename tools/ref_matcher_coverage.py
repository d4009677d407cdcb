"""What the scenes of tests/test_ref_matcher.py reach inside the reference's src/ORBmatcher.cc and src/MapPoint.cc.

Builds a third, --coverage -O0 variant of the reference matcher library (oracle/ref/build_ref.py's recipe) into a temporary
directory, replays every CPU case into it in a child process, runs gcov on the two sources and writes
profiles/ref_matcher_coverage.md: per function the executable lines run / not run and, for the matcher's entry points, every
line that no scene executed (a missed `continue`, `break`, `return`, `if` or `else` body), with the reason.  Line numbers and counts only: no reference
text is written.  CPU only; the figures are a record, not a gate.

    python tools/ref_matcher_coverage.py [--out profiles/ref_matcher_coverage.md]"""
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPLAY = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_ref_matcher as T
from compat_scenes import Harness
H = Harness(%r)
for cid in T.CPU_CASES + T.MODEL_CASES:
    T.play(cid, H, "strict")
"""
# why a line of the listed kind cannot run behind the stand-ins (oracle/ref/matcher/): matched by what the line tests
REASONS = [(r"isBad\(\)", "a bad MapPoint in a keyframe slot (SetBadFlag empties the slots of its observers and the harness fills slots only through AddObservation), or KeyFrame::isBad(), which is always false in the stand-in"),
           (r"!pMP|pMP\s*==\s*NULL|!pMP[12]", "a NULL MapPoint in the list")]


def main():
    from oracle.ref import build_ref as B
    out_md = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ref_matcher_coverage.md")
    if not B.reference_present():
        sys.exit("reference tree not found at %s" % B.reference_dir())
    with tempfile.TemporaryDirectory(prefix="ref_matcher_cov_") as d:
        so = os.path.join(d, "libref_matcher_cov.so")
        p = subprocess.run(B.matcher_command("strict", so, extra=["-O0", "--coverage"]), capture_output=True, text=True, cwd=d)
        if p.returncode:
            sys.exit(p.stderr[-4000:])
        subprocess.run([sys.executable, "-c", REPLAY % (ROOT, os.path.join(ROOT, "tests"), so)], check=True, cwd=d)
        report = []
        for src in ("ORBmatcher", "MapPoint"):
            subprocess.run(["gcov", "--json-format", os.path.basename(so) + "-" + src + ".gcno"], check=True, cwd=d, capture_output=True)
            with gzip.open(os.path.join(d, os.path.basename(so) + "-" + src + ".gcov.json.gz"), "rt") as f:
                data = json.load(f)
            ref_src = os.path.join(B.reference_dir(), "src", src + ".cc")
            text = open(ref_src, encoding="utf-8", errors="replace").read().split("\n")
            for fl in data["files"]:
                if os.path.basename(fl["file"]) != src + ".cc":
                    continue
                lines = {l["line_number"]: l["count"] for l in fl["lines"]}
                for fn in sorted(fl["functions"], key=lambda f: f["start_line"]):
                    a, b = fn["start_line"], fn["end_line"]
                    mine = {n: c for n, c in lines.items() if a <= n <= b}
                    missed = sorted(n for n, c in mine.items() if c == 0)
                    # every line of the matcher that did not run is a missed branch outcome (a `continue`, `break`, `return`, the
                    # body of an `if` or of an `else`): each is listed with the reason, or as reachable and not reached
                    why = []
                    for n in (missed if src == "ORBmatcher" else []):
                        # the condition guarding the line: the line itself or the nearest `if` above it
                        ctx = " ".join(t.split("//")[0] for t in text[max(a, n - 3) - 1:n])
                        code = text[n - 1].split("//")[0].strip()
                        if lines.get(n - 1, 0) and not text[n - 2].split("//")[0].rstrip().endswith((";", "{", "}")) and not re.search(r"\b(if|else)\b", text[n - 2]):
                            why.append((n, "a continuation line of the statement of line %d, which ran" % (n - 1)))
                        elif not code:
                            continue
                        else:
                            why.append((n, next((r for pat, r in REASONS if re.search(pat, ctx)), "REACHABLE, and not reached by any scene")))
                    report.append((src + ".cc", fn["demangled_name"].split("(")[0], a, b, fn["execution_count"], len(mine), len(mine) - len(missed), missed, why))
    with open(out_md, "w") as f:
        f.write("# Reference matcher coverage of the CPU scenes\n\n")
        f.write("Written by `tools/ref_matcher_coverage.py`: the reference's `src/ORBmatcher.cc` and `src/MapPoint.cc`, compiled unmodified with\n"
                "`-O0 --coverage` behind the stand-ins of `oracle/ref/matcher/`, after every CPU case of `tests/test_ref_matcher.py` was replayed.\n"
                "Line numbers refer to the reference's files; no reference text is reproduced.  A record, not a gate.\n\n")
        f.write("| file | function | lines | calls | executable | executed | not executed |\n|---|---|---|---|---|---|---|\n")
        for src, name, a, b, calls, n, hit, missed, why in report:
            f.write("| %s | `%s` | %d-%d | %d | %d | %d | %s |\n" % (src, name, a, b, calls, n, hit, " ".join(map(str, missed)) or "-"))
        f.write("\n## Lines of the matcher's methods that no scene executed, each a missed branch outcome\n\n")
        for src, name, a, b, calls, n, hit, missed, why in report:
            if why and calls:
                f.write("* `%s` (%s:%d): " % (name, src, a) + "; ".join("%d: %s" % w for w in why) + "\n")
        never = [r for r in report if not r[4]]
        if never:
            f.write("\n## Functions never called\n\n")
            for src, name, a, b, *_ in never:
                f.write("* `%s` (%s:%d-%d)\n" % (name, src, a, b))
    print(out_md)


if __name__ == "__main__":
    main()
