"""ORBX_PYRAMID_UPSTREAM on the host: the geometry of csrc/orbx_geometry.cpp under AddressSanitizer + UBSan against the Python
model (tests/upstream_model.py), and handle creation through the C ABI (host-only handles, no GPU)."""
import os
import subprocess

import pytest

import upstream_model as um
from orb_slam2_detailed_comments_amd import _capi, ORBextractor, OrbxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(640, 480), (752, 480), (1241, 376), (300, 200), (160, 120)]


@pytest.fixture(scope="module")
def san_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "san_geometry_upstream")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_geometry_upstream.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_geometry.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "FAIL" not in p.stdout, p.stdout[-3000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-3000:]
    return p.stdout.splitlines()


def _parse(lines):
    levels, totals, errors, cur = {}, {}, {}, None
    for ln in lines:
        t = ln.split()
        if t[0] == "G":
            v = [int(x) for x in t[1:]]
            cur = levels.setdefault((v[0], v[1]), {}).setdefault(v[2], dict(zip(
                ("sw", "sh", "qt_w", "qt_h", "nini", "kp_cap", "ncols", "nrows", "wcell", "hcell", "ncells"), v[3:])))
            cur["cells"] = []
        elif t[0] == "C":
            cur["cells"].append(tuple(int(x) for x in t[1:]))
        elif t[0] == "T":
            totals[(int(t[1]), int(t[2]))] = int(t[3])
        elif t[0] == "E":
            errors[(int(t[1]), int(t[2]), int(t[3]))] = (int(t[4]), " ".join(t[5:]))
    return levels, totals, errors


@pytest.mark.parametrize("w,h", SIZES)
def test_geometry_equals_the_model(san_output, w, h):
    levels, totals, _ = _parse(san_output)
    model = um.geometry(w, h, padded=False)
    assert sorted(levels[(w, h)]) == list(range(8))
    for l, m in enumerate(model):
        g = levels[(w, h)][l]
        for key in ("sw", "sh", "qt_w", "qt_h", "nini", "kp_cap"):
            assert g[key] == m[key], (l, key, g[key], m[key])
        cells = [c for c in m["cells"] if c[2] >= 7 and c[3] >= 7]     # cv::FAST yields nothing below 7 x 7: not tabled
        assert g["ncells"] == len(cells) and g["cells"] == cells, "cell table of level %d" % l
        if m["cells"]:
            assert (g["ncols"], g["nrows"], g["wcell"], g["hcell"]) == (m["ncols"], m["nrows"], m["wcell"], m["hcell"])
        for (x0, y0, cw, ch, _, _) in g["cells"]:                       # inside the view, 16 px from its edge
            assert 16 <= x0 and x0 + cw <= m["sw"] - 16 and 16 <= y0 and y0 + ch <= m["sh"] - 16
    assert totals[(w, h)] == sum(m["kp_cap"] for m in model)


def test_undefined_geometries_are_refused_by_name(san_output):
    _, _, errors = _parse(san_output)
    st, why = errors[(200, 96, 8)]
    assert st == _capi.UNSUPPORTED and "level 6" in why and "67 x 32" in why
    st, why = errors[(97, 131, 8)]
    assert st == _capi.BAD_ASPECT and "nIni" in why
    assert errors[(97, 131, 4)][0] == 0


@pytest.mark.parametrize("w,h", SIZES)
def test_max_keypoints_of_a_host_only_upstream_handle(built_lib, w, h):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2, pyramid_mode=_capi.PYRAMID_UPSTREAM)
    assert ex.max_keypoints(w, h) == sum(m["kp_cap"] for m in um.geometry(w, h, padded=False))


def test_handle_creation(built_lib):
    """fails on the parent: orbx_create answered every mode but the fork's with ORBX_UNSUPPORTED"""
    assert (_capi.PYRAMID_FORK_PADDED, _capi.PYRAMID_UPSTREAM) == (0, 1)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2, pyramid_mode=_capi.PYRAMID_UPSTREAM)     # check() raises unless ORBX_OK
    assert ex.params.pyramid_mode == 1 and ex.GetLevels() == 8
    with pytest.raises(OrbxError) as e:
        ORBextractor(1000, 1.2, 8, 20, 7, device=-2, pyramid_mode=2)
    assert e.value.status == _capi.UNSUPPORTED
    with pytest.raises(OrbxError) as e:
        ex.max_keypoints(200, 96)
    assert e.value.status == _capi.UNSUPPORTED and "level 6" in str(e.value)
    with pytest.raises(OrbxError) as e:
        ex.max_keypoints(97, 131)
    assert e.value.status == _capi.BAD_ASPECT
    assert ORBextractor(1000, 1.2, 8, 20, 7, device=-2).max_keypoints(200, 96) > 0               # the fork's region is 38 px larger


@pytest.mark.parametrize("mode", ["ORBX_PYRAMID_UPSTREAM", "ORBX_PYRAMID_FORK_PADDED"])
def test_compat_shim_takes_the_mode_at_compile_time(mode):
    """compat/ORBextractor.h with -DORBX_COMPAT_PYRAMID_MODE=...: parses and type-checks against tests/compat_stubs/, and the
    constructor hands the macro to orbx_create"""
    stubs = os.path.join(ROOT, "tests", "compat_stubs")
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-DORBX_COMPAT_PYRAMID_MODE=" + mode, "-I" + stubs,
                        "-I" + os.path.join(ROOT, "compat"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(stubs, "driver_extractor.cpp")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]
    src = open(os.path.join(ROOT, "compat", "ORBextractor.h")).read()
    assert "p.pyramid_mode = ORBX_COMPAT_PYRAMID_MODE;" in src and "#define ORBX_COMPAT_PYRAMID_MODE ORBX_PYRAMID_FORK_PADDED" in src
