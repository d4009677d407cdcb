"""orbx_search_by_sim3_batch on the device (k_grid_build over the pool, k_sim3s_project, k_sim3s_cand, k_sim3s_mutual) against the
library's host path (ORBX_SIM3SEARCH=host on the same handle) and tests/sim3_search_model.py, on the scenes of the CPU tests:
matches, counts and every debug field, exact equality, in both fp_modes.  Also: the recorded outputs of the reference's compiled
ORBmatcher.cc (tests/golden/sim3_search_*.json; the reference tree is not read); each problem of a batched call against the same
problem called alone and against the single orbx_search_by_sim3 fed the model's projections; a second call on the same handle
with a larger pool (staging and arena growth).  The scenes and the model's answers are computed once per process."""
import json
import os

import numpy as np
import pytest

import sim3_search_model as sm
import sim3_search_scenes as sc
from compat_scenes import target_dict
from orb_slam2_detailed_comments_amd import ORBextractor, ORBmatcher, _capi
from test_ref_matcher import entry
from test_sim3_search_cpu import FIELDS, GOLDEN, VARIANT, assert_equals_model, scenes_and_models, thresholds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[_capi.FP_GCC_FMA, _capi.FP_STRICT], ids=["fma", "strict"])
def ex(request):
    e = ORBextractor(1000, 1.2, 8, 20, 7, fp_mode=request.param)
    e.fp = request.param
    e.matcher = ORBmatcher(extractor=e)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def time_limit():
    """every test here is a GPU step with a limit of its own: a call that does not come back ends the process with a traceback"""
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def search(ex, s, problems=None, host=False, debug=True):
    if host:
        os.environ["ORBX_SIM3SEARCH"] = "host"
    try:
        return ex.matcher.SearchBySim3Batch(s["keyframes"], s["problems"] if problems is None else problems, s["camera4"], s["bounds4"],
                                            debug=debug)
    finally:
        os.environ.pop("ORBX_SIM3SEARCH", None)


def test_device_equals_host_path_equals_model_on_every_scene(ex):
    scenes, models = scenes_and_models(ex)
    for name, s in scenes.items():
        assert_equals_model(search(ex, s), models[name], name + ", device")
        assert_equals_model(search(ex, s, host=True), models[name], name + ", ORBX_SIM3SEARCH=host")
        counts, matches = search(ex, s, debug=False)                  # the short download
        assert counts == [m["n"] for m in models[name]] and all(np.array_equal(a, m["matches"]) for a, m in zip(matches, models[name]))


def test_device_reproduces_the_recorded_reference_outputs(ex):
    with open(GOLDEN % VARIANT[ex.fp]) as f:
        want = json.load(f)
    scenes, _ = scenes_and_models(ex)
    got = {}
    for name, s in scenes.items():
        counts, matches = search(ex, s, debug=False)
        for k in range(len(counts)):
            got["%s/%d" % (name, k)] = dict(n=counts[k], matches=entry(matches[k]))
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


def test_each_problem_alone_and_through_the_single_call(ex):
    scenes, models = scenes_and_models(ex)
    thr = thresholds(ex)
    for name in ("float", "shapes", "planted_selection"):
        s = scenes[name]
        inside = search(ex, s)
        for k, p in enumerate(s["problems"]):
            alone = search(ex, s, problems=[p])
            assert alone[0][0] == inside[0][k] and np.array_equal(alone[1][0], inside[1][k]), (name, k)
            for f in FIELDS:
                np.testing.assert_array_equal(alone[2][0][f], inside[2][k][f], err_msg="%s problem %d %s" % (name, k, f))
            k1, k2 = s["keyframes"][p["kf1"]], s["keyframes"][p["kf2"]]
            if len(k1["keys_un"]) == 0 or len(k2["keys_un"]) == 0:
                continue
            p12, p21, _ = sm.stage1(s, ex.fp == _capi.FP_GCC_FMA, thr, sc.scale_table(), k)
            n, m = ex.matcher.SearchBySim3(target_dict(k1["keys_un"], k1["desc"]), target_dict(k2["keys_un"], k2["desc"]), p12, p21, p["th"])
            assert n == inside[0][k] and np.array_equal(m, inside[1][k]), (name, k)


def test_a_second_call_with_a_larger_pool_on_the_same_handle(ex):
    """a fresh handle sees a small call first, then one whose pool, query count and download are several times larger (the
    staging block and the arena grow), then the small one again"""
    scenes, models = scenes_and_models(ex)
    e = ORBextractor(1000, 1.2, 8, 20, 7, fp_mode=ex.fp)
    e.matcher = ORBmatcher(extractor=e)
    try:
        small, large = scenes["planted_geometry"], scenes["float"]
        assert sum(len(k["keys_un"]) for k in large["keyframes"]) > 8 * sum(len(k["keys_un"]) for k in small["keyframes"])
        for name, s in (("planted_geometry", small), ("float", large), ("planted_geometry", small), ("float", large)):
            assert_equals_model(search(e, s), models[name], name + ", growing handle")
    finally:
        e.close()
