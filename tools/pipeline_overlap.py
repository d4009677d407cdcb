#!/usr/bin/env python3
"""How much of the pyramid's kernel time overlaps k_fast_rows / k_describe, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python bench.py --steps 10 --warmup 3
    python tools/pipeline_overlap.py OUT/**/run_kernel_trace.csv

Prints one JSON line: per kernel family the busy time (union of its launch intervals, ns), and the fraction of the pyramid's busy
time (k_pyr_l0* + k_pyr_resize*) during which a k_fast_rows / k_describe / k_quadtree launch was also running.  In the serial
sequence the fractions are ~0; in the sub-batch pipeline (ORBX_PIPELINE) they say how much of the pyramid ran hidden."""
import csv
import glob
import json
import sys


def union(iv):
    out = []
    for a, b in sorted(iv):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def overlap(u, v):
    i = j = 0
    tot = 0
    while i < len(u) and j < len(v):
        a, b = max(u[i][0], v[j][0]), min(u[i][1], v[j][1])
        if a < b:
            tot += b - a
        if u[i][1] < v[j][1]:
            i += 1
        else:
            j += 1
    return tot


def family(name):
    for f in ("k_pyr_l0", "k_pyr_resize", "k_fast_rows", "k_quadtree", "k_describe", "k_match"):
        if f in name:
            return "k_pyr" if f.startswith("k_pyr") else f
    return None


def main(paths):
    fams = {}
    for p in paths:
        for row in csv.DictReader(open(p)):
            f = family(row["Kernel_Name"])
            if f:
                fams.setdefault(f, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    u = {f: union(iv) for f, iv in fams.items()}
    busy = {f: sum(b - a for a, b in iv) for f, iv in u.items()}
    pyr = u.get("k_pyr", [])
    out = {"busy_ns": busy, "launches": {f: len(iv) for f, iv in fams.items()}}
    if busy.get("k_pyr"):
        for f in ("k_fast_rows", "k_describe", "k_quadtree"):
            out[f"pyr_overlap_{f}"] = round(overlap(pyr, u.get(f, [])) / busy["k_pyr"], 4)
        rest = union([iv for f in ("k_fast_rows", "k_describe", "k_quadtree") for iv in u.get(f, [])])
        out["pyr_overlap_any"] = round(overlap(pyr, rest) / busy["k_pyr"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    files = [f for a in sys.argv[1:] for f in glob.glob(a, recursive=True)]
    if not files:
        sys.exit("no kernel trace csv given")
    main(files)
