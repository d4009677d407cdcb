#!/usr/bin/env python3
"""Rates of the keyframe database (orbx_kfdb_query_reloc: steps 1-3 of KeyFrameDatabase::DetectRelocalizationCandidates) on
the device path (k_kfdb_common + k_kfdb_score) and on the library's own host path (the reference's inverted-file walk,
ORBX_KFDB=host) for the same database and the same queries, interleaved in one process.

Map: `entries` keyframes along a trajectory of entries / 10 places in a vocabulary of 10^6 words (ORBvoc.txt has 971 k); a
vector has ~1000 words, four fifths from its place's window of 2000 words (adjacent windows overlap by half), a fifth uniform.
Timed: the query call alone (upload of the queries, kernels, download of the sharers, the fold of the per-entry state);
steps 4-5 (orbx_kfdb_select_groups) are host code common to both paths and are left out.  One warm-up call per path, then
the median of `reps` interleaved calls, every call with fresh query ids.

    python tools/kfdb_rate.py [--entries 1000,10000,100000] [--queries 1,64,1024] [--reps R] [--md profiles/kfdb_rate.md]
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from orb_slam2_detailed_comments_amd import ORBextractor, KeyFrameDatabase, _capi

VOCAB, WORDS, WINDOW = 1000000, 1000, 2000


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def draw(rng, place):
    a = place * (WINDOW // 2) % (VOCAB - WINDOW) + rng.permutation(WINDOW)[:WORDS * 4 // 5]
    w = np.unique(np.concatenate([a, rng.integers(0, VOCAB, size=WORDS // 5)]).astype(np.uint32))
    v = rng.random(len(w)) + 0.05
    return w, v / v.sum()


def main():
    sizes = [int(x) for x in arg("--entries", "1000,10000,100000").split(",")]
    batches = [int(x) for x in arg("--queries", "1,64,1024").split(",")]
    reps = int(arg("--reps", "5"))
    md = arg("--md", "")
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=0)
    L, P = _capi.lib(), _capi.ptr
    rng = np.random.default_rng(7)
    rows = []
    next_id = [1]
    for N in sizes:
        places = max(N // 10, 1)
        db = KeyFrameDatabase(ex, scoring=0)
        t = time.perf_counter()
        for i in range(N):
            db.add(i, draw(rng, i % places))
        t_add = (time.perf_counter() - t) / N * 1e6
        for Q in batches:
            vs = [draw(rng, int(p)) for p in rng.integers(0, places, size=Q)]
            begin = np.zeros(Q + 1, np.int32); begin[1:] = np.cumsum([len(w) for w, _ in vs])
            qw = np.concatenate([w for w, _ in vs]); qv = np.concatenate([v for _, v in vs])
            nm = np.zeros(Q, np.int32); mc = np.zeros(Q, np.int32)

            def call(path):
                os.environ["ORBX_KFDB"] = path
                ids = np.arange(next_id[0], next_id[0] + Q, dtype=np.int64); next_id[0] += Q
                t0 = time.perf_counter()
                _capi.check(L.orbx_kfdb_query_reloc(db._h, Q, P(ids), P(begin), P(qw), P(qv), P(nm), P(mc)))
                return time.perf_counter() - t0, nm.copy(), mc.copy()

            ref = {}
            for path in ("device", "host"):
                _, ref[path + "_nm"], ref[path + "_mc"] = call(path)        # warm-up, and the two paths must agree
            assert np.array_equal(ref["device_nm"], ref["host_nm"]) and np.array_equal(ref["device_mc"], ref["host_mc"])
            r = max(2, reps if N * Q <= 10 ** 7 else 3)
            td, th = [], []
            for _ in range(r):
                td.append(call("device")[0]); th.append(call("host")[0])
            d, h = float(np.median(td)) / Q * 1e6, float(np.median(th)) / Q * 1e6
            rows.append((N, Q, d, min(td) / Q * 1e6, max(td) / Q * 1e6, h, min(th) / Q * 1e6, max(th) / Q * 1e6,
                         float(nm.mean()), t_add))
            print(f"entries {N:7d}  queries/call {Q:5d}  device {d:10.1f} us/query [{rows[-1][3]:.1f} .. {rows[-1][4]:.1f}]  "
                  f"host {h:10.1f} us/query [{rows[-1][6]:.1f} .. {rows[-1][7]:.1f}]  host/device {h / d:6.2f}x  "
                  f"scored/query {nm.mean():.1f}  add {t_add:.1f} us/entry", flush=True)
        del db
    os.environ.pop("ORBX_KFDB", None)
    if md:
        with open(md, "w") as f:
            f.write("# Keyframe database: relocalisation query, device path against the library's host path\n\n"
                    "`python tools/kfdb_rate.py` on one MI355X; microseconds per query (median of interleaved calls, range in\n"
                    "brackets), steps 1-3 only, ~1000-word vectors in a 10^6-word vocabulary, L1 scoring.  `host/device` > 1:\n"
                    "the device path is faster.\n\n"
                    "| entries | queries per call | device us/query | host us/query | host/device | entries scored per query |\n"
                    "|---:|---:|---:|---:|---:|---:|\n")
            for N, Q, d, dlo, dhi, h, hlo, hhi, sc, _ in rows:
                f.write(f"| {N} | {Q} | {d:.1f} [{dlo:.1f} .. {dhi:.1f}] | {h:.1f} [{hlo:.1f} .. {hhi:.1f}] | {h / d:.2f} | {sc:.1f} |\n")


if __name__ == "__main__":
    main()
