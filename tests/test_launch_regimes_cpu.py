"""The launchers' size rules (csrc/orbx_launch.h) through the debug exports, on a host-only handle: orbx_debug_match_plan and
orbx_debug_fast_gpw are pure arithmetic.  Every shape the GPU regime tests use (tests/test_match_regimes_gpu.py, tests/test_fast_net_gpu.py)
is in the regime it is meant for, the bench shape is QT = 4, the small shapes of the older parity tests are nsplit = 16 / one group
per wave, and ORBX_FAST_GPW is validated."""
import pytest
from orb_slam2_detailed_comments_amd import ORBextractor, OrbxError, _capi
import test_fast_net_gpu as fast
import test_match_regimes_gpu as regimes

ENV = {"mfma_fp4": None, "mfma_i8": "i8", "valu": "valu"}


def _handle(monkeypatch, kernel=None, gpw=None, **kw):
    for k, v in (("ORBX_MATCH_KERNEL", ENV[kernel] if kernel else None), ("ORBX_FAST_GPW", gpw)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    return ORBextractor(kw.pop("nfeatures", 300), device=-2, **kw)       # host-only: tables and arithmetic, no device work


def _rule_mfma(npairs, stride):
    """the rule as tests/test_match_regimes_gpu.py states it"""
    if -(-stride // 128) * npairs >= 2048:
        return 4, 1
    return 2, min(16, max(1, 4096 // (-(-stride // 64) * npairs)))


def _rule_valu(npairs, stride):
    base = -(-stride // 128) * npairs
    return 0, min(16, max(1, -(-16384 // base)))


@pytest.mark.parametrize("kernel", list(ENV))
def test_match_plan_of_every_tested_shape(kernel, built_lib, monkeypatch):
    ex = _handle(monkeypatch, kernel)
    rule = _rule_valu if kernel == "valu" else _rule_mfma
    cases = regimes.VALU_CASES if kernel == "valu" else regimes.MFMA_CASES
    for name, (npairs, stride, plan) in cases.items():
        assert regimes.match_plan(ex.handle, npairs, stride) == plan == rule(npairs, stride), name
    # the cases are the smallest launches of their regime: one pair less (QT = 4, the vector pipe's nsplit = 1) or one more
    # (a QT = 2 split count) is the neighbouring regime
    if kernel == "valu":
        assert regimes.match_plan(ex.handle, 16383, 8) == (0, 2) and regimes.match_plan(ex.handle, 5462, 8) == (0, 3)
    else:
        assert regimes.match_plan(ex.handle, 2047, 128) == (2, 1)
        assert regimes.match_plan(ex.handle, 1366, 64) == (2, 2) and regimes.match_plan(ex.handle, 586, 64) == (2, 6)
        assert regimes.match_plan(ex.handle, 2048, 64) == (4, 1) and regimes.match_plan(ex.handle, 2048, 100) == (4, 1)
    # the single-pair call at the packing limit and the shapes of tests/test_gpu_parity.py's matcher tests: the default regime
    small = [(1, n) for n in (3, 1, 63, 64, 65, 1000, 300, 5, 257, 33)] + [(7, 200), (40, 130)]
    for npairs, stride in small:
        assert regimes.match_plan(ex.handle, npairs, stride) == ((0, 16) if kernel == "valu" else (2, 16)) == rule(npairs, stride)
    # the bench shape: 1024 pairs, out_stride = the keypoint capacity of 640x480 at 1000 features
    cap = _handle(monkeypatch, kernel, nfeatures=1000).max_keypoints(640, 480)
    assert cap == 1024
    assert regimes.match_plan(ex.handle, 1024, cap) == ((0, 2) if kernel == "valu" else (4, 1))
    with pytest.raises(OrbxError):
        regimes.match_plan(ex.handle, 0, 64)
    with pytest.raises(OrbxError):
        regimes.match_plan(ex.handle, 8, 0)


def test_fast_gpw_size_rule_and_knob(built_lib, monkeypatch):
    l0, total = fast.group_counts(fast.W, fast.H)
    ex = _handle(monkeypatch)                                # knob unset: the size rule
    for b, ng in fast.fast_launches("slab", fast.NF, fast.W, fast.H) + fast.fast_launches("fastfirst", fast.NF, fast.W, fast.H) + \
            fast.fast_launches("inplace", fast.NF, fast.W_ODD, fast.H_ODD) + fast.fast_launches("fastfirst", fast.NF, fast.W_ODD, fast.H_ODD):
        assert fast.fast_gpw(ex, b, ng) == 1, (b, ng)        # the 16-frame planted batches: one group per wave unless forced
    assert fast.fast_gpw(ex, 400, total) == 2 and fast.fast_gpw(ex, 384, total) == 1     # test_size_rule_pairs_the_planted_groups
    assert fast.fast_gpw(ex, 1024, 16) == 2 and fast.fast_gpw(ex, 1023, 16) == 1         # frames x groups >= 16384
    assert fast.fast_gpw(ex, 1824, 9) == 2 and fast.fast_gpw(ex, 912, 18) == 2           # tests/test_fast_first_plan.py, 128x96
    assert fast.fast_gpw(ex, 256, 176) == 2 and fast.fast_gpw(ex, 128, 350) == 2         # ... and 640x480 x 256
    assert fast.fast_gpw(ex, 1 << 20, 1 << 20) == 2                                      # no 32-bit overflow in the product
    for forced in ("1", "2"):
        ex = _handle(monkeypatch, gpw=forced)
        for b, ng in ((16, total), (16, l0), (8, total - l0), (400, total), (1, 1)):
            assert fast.fast_gpw(ex, b, ng) == int(forced), (forced, b, ng)
    for bad in ("0", "3", "-1", "two", "", "2x", "16"):
        ex = _handle(monkeypatch, gpw=bad)
        with pytest.raises(OrbxError) as e:
            fast.fast_gpw(ex, 16, total)
        assert e.value.status == _capi.BAD_ARGUMENT and "ORBX_FAST_GPW" in str(e.value), bad
    ex = _handle(monkeypatch)
    with pytest.raises(OrbxError):
        fast.fast_gpw(ex, 0, total)
