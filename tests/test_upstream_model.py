"""tests/upstream_model.py with the padded switch IS the oracle: counts, all 28 keypoint bytes, descriptors and the per-level
stages equal OracleExtractor's, in both fp_modes.  That anchors the model to the oracle (itself pinned to the compiled
reference); the upstream switch then differs by the one line `mvImagePyramid[level] = temp;`."""
import glob
import os

import numpy as np
import pytest

import oracle.orb_oracle as oo
import ref_extractor as rx
import upstream_model as um

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _inputs():
    out = []
    for f in sorted(glob.glob(os.path.join(GOLD, "s*.npz"))):
        out.append((os.path.basename(f)[:-4], np.load(f)["image"]))
    out.append(("blocks300x200", um.block_image(3, 300, 200, 6)))
    out.append(("blocks640x480", um.block_image(4, 640, 480, 12)))
    return out


INPUTS = _inputs()


@pytest.mark.parametrize("fp", ["strict", "fma"])
@pytest.mark.parametrize("name", [n for n, _ in INPUTS])
def test_padded_model_is_the_oracle(name, fp):
    img = dict(INPUTS)[name]
    assert len(INPUTS) == 5
    nl = 8
    a = rx.cpu_stages(oo.OracleExtractor(fp_mode=rx.FP[fp]), img, nl)
    b = rx.cpu_stages(um.ModelExtractor(fp_mode=rx.FP[fp], padded=True), img, nl)
    assert a["n"] >= 0
    rx.assert_stages_equal(a, b, "%s/%s padded model against the oracle" % (name, fp))
    if a["n"] > 0:   # the blurred levels too (levels without keypoints are never blurred)
        E = oo.OracleExtractor(fp_mode=rx.FP[fp]); E.extract(img)
        M = um.ModelExtractor(fp_mode=rx.FP[fp], padded=True); M.extract(img)
        for l in range(nl):
            x, y = E.level_image(l, blur=True), M.level_image(l, blur=True)
            assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), "blurred level %d" % l


def test_upstream_switch_changes_what_a_level_is():
    """the view is the window at (19, 19) of the fork's level 0, and keypoints move to image coordinates"""
    img = dict(INPUTS)["s160x120"]
    F = um.ModelExtractor(padded=True); nf, kf, _ = F.extract(img)
    U = um.ModelExtractor(padded=False); nu, ku, _ = U.extract(img)
    assert np.array_equal(U.level_image(0), img) and np.array_equal(F.level_image(0)[19:-19, 19:-19], img)
    assert [a.shape for a in U.pyr] == [(s[1], s[0]) for s in um.level_sizes(160, 120, U.inv)]
    assert nu == 39
    k0 = ku[ku["octave"] == 0]
    assert k0["x"].min() >= 19 and k0["x"].max() < 160 - 19 and k0["y"].min() >= 19 and k0["y"].max() < 120 - 19


@pytest.mark.parametrize("w,h,nlevels,status,level", [(200, 96, 8, "UNSUPPORTED", 6), (97, 131, 8, "BAD_ASPECT", 4)])
def test_model_raises_on_undefined_geometry(w, h, nlevels, status, level):
    with pytest.raises(um.UndefinedGeometry) as e:
        um.ModelExtractor(nlevels=nlevels, padded=False).extract(um.block_image(5, w, h, 6))
    assert (e.value.status, e.value.level) == (status, level)
    with pytest.raises(um.UndefinedGeometry):
        um.geometry(w, h, nlevels=nlevels)
