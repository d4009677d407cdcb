"""Initializer H / F RANSAC on the device (orbx_init_ransac_batch_create: k_init_hypotheses, k_init_scores) against the library's
host path (ORBX_INIT=host on the same handle) and tests/init_model.py, on the scenes of the CPU tests.  Every comparison is
exact: T1 and T2, every hypothesis matrix and inverse, every score and RH as uint32, every mask, the best iterations, the model.
Both fp_modes run the same scenes and must give the same bits.

Sizes: n in {8, 9, 63, 64, 65, 129} (the minimal set, mask word boundaries and the tail) and {255, 256, 257} (the LDS chunk of
k_init_scores); iterations in {1, 200} and {63, 64, 65}: k_init_hypotheses runs ORBX_INIT_HYP_LANES = 64 hypotheses per workgroup
over ALL hypotheses of the call and k_init_scores 64 hypotheses of one problem per workgroup, so with both models the H / F
boundary of a problem falls inside a workgroup and the mixed call puts problem boundaries inside one; H only, F only and both;
n1 != n2, both larger than n.  Problems of different n, iteration counts and models are mixed in one call with two that launch
nothing, at most 16 problems per call, and no problem at all.  The model's answers are computed once per process
(tests/init_scenes.py)."""
import os

import pytest

import init_model as im
import init_scenes as sc
from orb_slam2_detailed_comments_amd import InitializerRansac, ORBextractor, _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[_capi.FP_GCC_FMA, _capi.FP_STRICT], ids=["fma", "strict"])
def ex(request):
    e = ORBextractor(1000, 1.2, 8, 20, 7, fp_mode=request.param)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def time_limit():
    """every test here is a GPU step with a limit of its own: a call that does not come back ends the process with a traceback"""
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def check(ex, problems, what):
    """device = model, then ORBX_INIT=host on the same handle = model"""
    assert len(problems) <= 16
    for env in (None, "host"):
        if env:
            os.environ["ORBX_INIT"] = env
        try:
            rb = InitializerRansac(ex, problems)
        finally:
            os.environ.pop("ORBX_INIT", None)
        try:
            sc.assert_batch_equals_model(rb, problems, f"{what}, ORBX_INIT={env}")
        finally:
            rb.close()


def test_size_list_device_equals_host_path_equals_model(ex):
    probs = list(sc.size_problems())
    assert set(sc.GPU_N) <= {len(p["matches"]) for p in probs} and set(sc.GPU_ITERATIONS) <= {p["iterations"] for p in probs}
    assert {p["models"] for p in probs} == {im.H, im.FUND, im.H | im.FUND}
    assert all(len(p["keys1"]) != len(p["keys2"]) and min(len(p["keys1"]), len(p["keys2"])) >= len(p["matches"]) for p in probs)
    assert any(len(p["keys1"]) > len(p["matches"]) < len(p["keys2"]) for p in probs)
    check(ex, probs[:9], "n")
    check(ex, probs[9:], "iterations")
    for p in probs[11:14]:                                      # the workgroup boundary of k_init_hypotheses, each alone
        check(ex, [p], f"hypothesis partition {p['iterations']}")


def test_mixed_call_with_problems_that_launch_nothing_and_no_problem_at_all(ex):
    mixed = sc.mixed_call()
    assert len(mixed) <= 16 and sum(not sc.launches(p) for p in mixed) == 2
    check(ex, mixed, "mixed")
    check(ex, [mixed[1], mixed[3]], "nothing launches")
    rb = InitializerRansac(ex, [])
    assert len(rb) == 0
    rb.close()
    for k, p in enumerate(mixed):                              # a problem alone gives what it gives inside the batch
        check(ex, [p], f"single {k}")


def test_planted_degenerate_and_none_scenes(ex):
    check(ex, list(sc.planted_scenes()), "planted")
    check(ex, [sc.degenerate()] + list(sc.none_scenes()), "degenerate, none")
    rb = InitializerRansac(ex, list(sc.none_scenes()))
    try:
        assert [rb.result(k)["model"] for k in range(3)] == [im.NONE] * 3
    finally:
        rb.close()
