"""The row walk of the pyramid resize (csrc/orbx_kernels.hip rr_walk: k_pyr_resize_rows and k_pyr_resize_rows_l1).  The walk
takes two destination rows per step and two steps per trip of its loop, keeps the rows of the next step in flight in a second
register set and fetches the vertical tap records of a row pair with one scalar load.  It changes how the bytes are computed,
not the bytes: every level of every frame must equal, byte for byte, (a) the oracle's level image (the upstream model's in
upstream mode) and (b) the same library run with ORBX_RESIZE_IMPL=legacy (k_pyr_resize, the second implementation).

ORBX_RR_RPW forces the destination rows per wave, so batches of two or three small frames reach every trip shape: row ranges
of 1, 2, 3, 4, 5 and 7 rows at the end of a level (ph mod rpw), ranges that end after the first or the second step of a trip,
and the record beyond the last row of a level of odd height.  The sizes were found with tests/resize_rows_geometry.cpp (the
geometry builder on the CPU); test_the_cases_have_the_shapes_they_are_there_for checks on the CPU that they still have them."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from orb_slam2_detailed_comments_amd import ORBextractor, synth, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

KNOBS = ("ORBX_RR_RPW", "ORBX_RESIZE_IMPL", "ORBX_LEVEL0_INPLACE", "ORBX_PLAN", "ORBX_PLAN_SUB", "ORBX_PLAN_HEAD", "ORBX_PLAN_MIN_FRAMES",
         "ORBX_PIPELINE", "ORBX_PIPELINE_HEAD", "ORBX_FAST_ROOM", "ORBX_FORK_LEVEL")
RPWS = (2, 4, 8, 16, 32)
NF = 200

# name: (width, height, stride, scale factor, nlevels, frames).  Level-1 width pw and height ph (padded) in the comments.
CASES = {
    "pw256_rows1": (262, 71, 264, 1.2, 8, 2),     # pw 256 = one full strip; ph 97: a last range of 1 row for every rpw
    "pw257_rows3": (263, 73, 264, 1.2, 8, 2),     # pw 257: ONE active lane in the last strip; ph 99: 3 rows (rpw >= 4)
    "pw255_rows5": (260, 76, 260, 1.2, 8, 3),     # pw 255; ph 101: 5 rows (rpw >= 8), 1 row (rpw 4)
    "pw253_rows7": (258, 78, 272, 1.2, 8, 2),     # pw 253; ph 103: 7 rows (rpw >= 8); stride > width
    "pw260_rows4": (266, 74, 268, 1.2, 8, 2),     # pw 260: one full dword in the last strip; ph 100: 4 rows (rpw >= 8)
    "body_tail_rows2": (320, 72, 320, 1.2, 8, 2),  # level 1 in place: strip 0 reads 12-byte windows, strip 1 is a tail strip; ph 98: 2 rows
    "three_levels": (262, 71, 264, 1.2, 3, 2),
    "scale_1_1": (262, 70, 264, 1.1, 8, 2),       # most destination rows re-use a filtered source row
    "scale_1_5": (262, 70, 264, 1.5, 8, 2),
    "scale_1_5_three_levels": (262, 70, 264, 1.5, 3, 2),
    "scale_2_0": (262, 70, 264, 2.0, 8, 2),       # never re-uses a filtered row; its level-1 raw table is rejected: eager level 0
}
# tap records of the rows and columns of every level (tests/resize_rows_geometry.cpp: FNV-1a), as the geometry builder gave them
# BEFORE the vertical tables got their record beyond the last row: the records a row names have not moved or changed
TAP_HASH = {
    (640, 480, 1.2, 8, 0): "3daacd1e4c5b8a4b",
    (262, 70, 1.1, 8, 0): "ad4329f4542d861b", (262, 70, 1.1, 3, 0): "779a51d3b5ce09bc", (262, 70, 1.5, 8, 0): "1f5389f4ec5844ec",
    (262, 70, 1.5, 3, 0): "404c6d9357256143", (262, 70, 2.0, 8, 0): "908ed6cd59169a45", (262, 70, 2.0, 3, 0): "ce212319b5d354bd",
    (300, 200, 1.2, 8, 1): "1fa5ce26d61900d3", (300, 200, 1.2, 3, 1): "d067b11a7dae0756",
}
UPSTREAM = (300, 200, 300, 1.2)   # the smallest shape tests/test_upstream_gpu.py runs with eight levels that all have a region


# ------------------------------------------------------------------------------------------------------------ CPU

@functools.lru_cache(maxsize=None)
def _geometry_tool():
    import tempfile
    d = tempfile.mkdtemp(prefix="rrgeo")
    exe = os.path.join(d, "resize_rows_geometry")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "resize_rows_geometry.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_geometry.cpp"), "-o", exe])
    return exe


def _geometries(keys):
    """{(w, h, sf, nl, upstream): dict(l1_inplace, l1_tail_bx, hash, levels=[(pw, ph)])}; fails on any FAIL line of the tool"""
    args = []
    for k in keys:
        args += [str(v) for v in k]
    p = subprocess.run([_geometry_tool()] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "FAIL" not in p.stdout, p.stdout[-3000:] + p.stderr[-1000:]
    out, cur = {}, None
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] == "geo":
            assert int(f[7]) == 0, line
            cur = dict(l1_inplace=int(f[9]), l1_tail_bx=int(f[11]), taps=int(f[13]), hash=f[15], levels=[])
            out[(int(f[1]), int(f[2]), float(f[3]), int(f[4]), int(f[5]))] = cur
        elif f[0] == "level":
            cur["levels"].append((int(f[2]), int(f[3])))
    assert len(out) == len(set(keys))
    return out


def _key(case, up=0):
    w, h, _, sf, nl, _ = CASES[case]
    return (w, h, sf, nl, up)


def test_record_beyond_the_last_row_is_no_tap_of_a_row(built_lib):
    """the vertical tap tables carry one more record (the row walk reads the records of rows Y, Y + 1 together): the tool fails
    unless that record exists, repeats the last row's, and lies in no level's range; the records of the rows and columns hash to
    what they hashed to before the tables were padded; and the host tables tests/test_abi.py compares are the oracle's"""
    keys = list(TAP_HASH) + [_key(c) for c in CASES]
    geo = _geometries(keys)
    for k, h in TAP_HASH.items():
        assert geo[k]["hash"] == h, (k, geo[k]["hash"])
    g = geo[(640, 480, 1.2, 8, 0)]
    rows = sum(pw + ph for pw, ph in g["levels"][1:]) + sum(g["levels"][1])     # seven levels + the raw-coordinate level-1 table
    assert g["taps"] == rows + 8, (g["taps"], rows)                            # one more record per vertical table, nothing else
    for nf, sf, nl in ((1000, 1.2, 8), (500, 1.5, 4)):
        ex = ORBextractor(nf, sf, nl, 20, 7, device=-2)
        t = oracle.OracleExtractor(nf, sf, nl).tables()
        assert np.array_equal(ex.GetScaleFactors(), t["scale"]) and np.array_equal(ex.GetInverseScaleFactors(), t["inv_scale"])
        assert np.array_equal(ex.GetScaleSigmaSquares(), t["sigma2"]) and np.array_equal(ex.GetInverseScaleSigmaSquares(), t["inv_sigma2"])
        assert np.array_equal(ex.features_per_level(), t["features_per_level"]) and np.array_equal(ex.umax(), t["umax"])
    assert ORBextractor(1000, 1.2, 8, 20, 7, device=-2).max_keypoints(640, 480) == sum(max(n + 3, 4) for n in [217, 181, 151, 126, 105, 87, 73, 60])


def test_the_cases_have_the_shapes_they_are_there_for(built_lib):
    geo = _geometries([_key(c) for c in CASES] + [UPSTREAM[:2] + (1.2, 8, 1)])
    l1 = lambda c: geo[_key(c)]["levels"][1]
    # strip shapes of level 1
    assert l1("pw256_rows1")[0] % 256 == 0 and l1("pw257_rows3")[0] % 256 == 1 and l1("pw260_rows4")[0] % 256 == 4
    assert l1("pw255_rows5")[0] % 256 == 255 and l1("pw253_rows7")[0] % 256 == 253
    for c in CASES:
        g, (w, h, stride, sf, nl, b) = geo[_key(c)], CASES[c]
        assert bool(g["l1_inplace"]) == (sf != 2.0) and stride % 4 == 0 and stride >= w and b in (2, 3), c
    g = geo[_key("body_tail_rows2")]
    assert 0 < g["l1_tail_bx"] < (g["levels"][1][0] + 255) // 256          # body strips and tail strips in one launch
    assert geo[_key("pw257_rows3")]["l1_tail_bx"] == 0                      # every strip a tail strip
    assert CASES["pw253_rows7"][2] > CASES["pw253_rows7"][0] + 8           # stride > width
    # trip shapes: rows of the last range of a level = ph mod rpw, for the in-place level-1 kernel (level 1 of a case whose raw
    # table passed) and for the slab kernel (levels >= 2, and level 1 of the eager runs)
    want = {1, 2, 3, 4, 5, 7}
    l1_rows = {l1(c)[1] % r for c in CASES for r in RPWS if geo[_key(c)]["l1_inplace"]}
    slab_rows = {ph % r for c in CASES for pw, ph in geo[_key(c)]["levels"][1:] for r in RPWS}
    assert want <= l1_rows and want <= slab_rows, (sorted(l1_rows), sorted(slab_rows))
    for c, rows in (("pw256_rows1", 1), ("pw257_rows3", 3), ("pw255_rows5", 5), ("pw253_rows7", 7), ("pw260_rows4", 4), ("body_tail_rows2", 2)):
        assert l1(c)[1] % 32 == rows and l1(c)[1] % 8 == rows % 8, c
    assert any(ph % 2 for c in CASES for pw, ph in geo[_key(c)]["levels"][1:])   # odd heights: the record beyond the last row is read
    # every rpw leaves some level with more than one range per strip, and rpw = 2 with ranges that end after one step
    assert all(ph > 32 for c in CASES for pw, ph in geo[_key(c)]["levels"][1:])
    up = geo[UPSTREAM[:2] + (1.2, 8, 1)]
    assert want & {ph % r for pw, ph in up["levels"][1:] for r in RPWS} >= {1, 2, 5}


# ------------------------------------------------------------------------------------------------------------ GPU

@functools.lru_cache(maxsize=None)
def _frames(w, h, b, stream_id):
    f = synth.stream(w, h, b, stream_id=stream_id)
    f.setflags(write=False)
    return f


def _run(monkeypatch, env, frames, stride, sf, nl, levels_of=None, pyramid_mode=_capi.PYRAMID_FORK_PADDED, nf=NF, outputs=False):
    """fresh handle under `env`, one device-pointer call; {(level, frame): image} (and the output arrays)"""
    import torch
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    b, h, w = frames.shape
    host = np.full((b, h, stride), 0xEE, np.uint8)
    host[:, :, :w] = frames
    dev = torch.device("cuda", 0)
    ex = ORBextractor(nf, sf, nl, 20, 7, max_batch=b, pyramid_mode=pyramid_mode)
    cap = ex.max_keypoints(w, h)
    imgs = torch.from_numpy(host).to(dev)
    out = dict(kps=torch.full((b, cap * 28), 0xA5, dtype=torch.uint8, device=dev), desc=torch.full((b, cap * 32), 0x5A, dtype=torch.uint8, device=dev),
               cnt=torch.full((b,), -3, dtype=torch.int32, device=dev), st=torch.full((b,), -5, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ex.extract_batch_device(imgs, b, w, h, stride, h * stride, out["kps"], out["desc"], out["cnt"], out["st"], cap)
    ex.synchronize()
    assert not out["st"].cpu().numpy().any(), env
    pyr = {(l, f): ex.pyramid_level(l, f) for f in (range(b) if levels_of is None else levels_of) for l in range(nl)}
    res = {k: v.cpu().numpy() for k, v in out.items()} if outputs else None
    ex.close()
    del imgs
    return (pyr, res) if outputs else pyr


@functools.lru_cache(maxsize=None)
def _oracle_levels(case):
    w, h, _, sf, nl, b = CASES[case]
    fr = _frames(w, h, b, 700 + len(case))
    ref = {}
    for f in range(b):
        orc = oracle.OracleExtractor(NF, sf, nl)
        orc.extract(np.ascontiguousarray(fr[f]))
        for l in range(nl):
            ref[(l, f)] = orc.level_image(l).copy()
    return ref


def _assert_levels(got, ref, what):
    assert got.keys() == ref.keys()
    for key in sorted(ref):
        assert got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), f"{what}: level {key[0]} of frame {key[1]} differs"


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_every_level_equals_oracle_and_legacy_for_every_rpw(monkeypatch, case):
    """in place (the default; level 1 by k_pyr_resize_rows_l1) and eager (every level by k_pyr_resize_rows), the launcher's own
    choice and rpw forced to 2, 4, 8, 16, 32"""
    w, h, stride, sf, nl, b = CASES[case]
    fr = _frames(w, h, b, 700 + len(case))
    ref = _oracle_levels(case)
    legacy = _run(monkeypatch, {"ORBX_RESIZE_IMPL": "legacy"}, fr, stride, sf, nl)
    _assert_levels(legacy, ref, f"{case}: legacy kernel against the oracle")
    for mode in ({}, {"ORBX_LEVEL0_INPLACE": "0"}):
        for rpw in (None,) + RPWS:
            env = dict(mode, **({} if rpw is None else {"ORBX_RR_RPW": rpw}))
            got = _run(monkeypatch, env, fr, stride, sf, nl)
            _assert_levels(got, ref, f"{case} {env}: against the oracle")
            _assert_levels(got, legacy, f"{case} {env}: against ORBX_RESIZE_IMPL=legacy")


@gpu
@pytest.mark.parametrize("nl", [8, 3])
def test_upstream_mode_equals_model_and_legacy_for_every_rpw(monkeypatch, nl):
    import upstream_model as um
    w, h, stride, sf = UPSTREAM
    fr = _frames(w, h, 2, 760)
    ref = {}
    for f in range(2):
        M = um.ModelExtractor(NF, sf, nl, 20, 7, padded=False)
        M.compute_pyramid(np.ascontiguousarray(fr[f]))
        for l in range(nl):
            ref[(l, f)] = np.ascontiguousarray(M.pyr[l])
    UP = _capi.PYRAMID_UPSTREAM
    legacy = _run(monkeypatch, {"ORBX_RESIZE_IMPL": "legacy"}, fr, stride, sf, nl, pyramid_mode=UP)
    _assert_levels(legacy, ref, "upstream: legacy kernel against the model")
    for rpw in (None,) + RPWS:
        env = {} if rpw is None else {"ORBX_RR_RPW": rpw}
        got = _run(monkeypatch, env, fr, stride, sf, nl, pyramid_mode=UP)
        _assert_levels(got, ref, f"upstream {env}: against the model")
        _assert_levels(got, legacy, f"upstream {env}: against ORBX_RESIZE_IMPL=legacy")


@gpu
def test_256_small_frames_fast_first_plan_against_serial(monkeypatch):
    """the resize chains of the sub-batches on the side stream beside FAST: outputs and levels equal the serial sequence's"""
    w, h, nf = 96, 80, 300
    frames = _frames(w, h, 8, 770)[np.arange(256) % 8]
    serial, sres = _run(monkeypatch, {"ORBX_PLAN": "serial"}, frames, w, 1.2, 8, levels_of=(0, 129, 255), nf=nf, outputs=True)
    assert (sres["cnt"] > 0).all()
    orc = oracle.OracleExtractor(nf)
    orc.extract(np.ascontiguousarray(frames[255]))
    for l in range(8):
        assert np.array_equal(serial[(l, 255)], orc.level_image(l)), f"serial sequence: level {l} differs from the oracle"
    for more in ({}, {"ORBX_RR_RPW": 4}, {"ORBX_RR_RPW": 32}):
        env = dict({"ORBX_PLAN": "fastfirst", "ORBX_PLAN_MIN_FRAMES": 8, "ORBX_PLAN_SUB": 2}, **more)
        got, res = _run(monkeypatch, env, frames, w, 1.2, 8, levels_of=(0, 129, 255), nf=nf, outputs=True)
        _assert_levels(got, serial, f"{env}: against ORBX_PLAN=serial")
        for k in sres:
            assert res[k].tobytes() == sres[k].tobytes(), f"{env}: {k} differs from the serial sequence"


@gpu
def test_rpw_knob_rejects_what_the_walk_cannot_take(monkeypatch):
    """rows per wave must be even (rows are taken in pairs) and a power of two in 2..64"""
    from orb_slam2_detailed_comments_amd import OrbxError
    fr = _frames(96, 80, 8, 770)[:2]
    for bad in ("1", "3", "12", "128", "0"):
        with pytest.raises(OrbxError):
            _run(monkeypatch, {"ORBX_RR_RPW": bad}, fr, 96, 1.2, 8)
