"""PnPsolver RANSAC on the device (orbx_pnp_ransac_batch_create: k_pnp_hypotheses, k_pnp_inliers) against the library's host path
(ORBX_PNP=host on the same handle) and tests/pnp_model.py, on the scenes of the CPU tests.  Every comparison is exact: the
double R and t equal as uint64, the float Tcw as uint32, the chosen N, masks, counts, every iterate return and the best state
after every call.  Both fp_modes run the same scenes and must give the same bits.

Sizes: N in {4, 5, 63, 64, 65, 129} (the minimal set, mask word boundaries and the tail) and {511, 512, 513} (the LDS chunk of
k_pnp_inliers); iterations in {1, 5, 35, 64, 65, 300} (wave and workgroup boundaries of k_pnp_inliers, which takes 4 iterations
per workgroup) and {31, 32, 33}: k_pnp_hypotheses runs ORBX_PNP_HYP_LANES = 32 hypotheses per workgroup, one per lane of half a
wave, over ALL iterations of the call, so the mixed calls also put problem boundaries inside a workgroup.  Problems of different
N and iteration counts are mixed in one call with some that launch nothing, at most 16 problems per call, and no problem at all.
The model's answers are computed once per process (tests/pnp_scenes.py)."""
import os

import numpy as np
import pytest

import pnp_scenes as ps
from orb_slam2_detailed_comments_amd import ORBextractor, PnPRansac, _capi

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


def check(ex, problems, what, replay=True):
    """device = model, then ORBX_PNP=host on the same handle = model"""
    assert len(problems) <= 16
    for env in (None, "host"):
        if env:
            os.environ["ORBX_PNP"] = env
        try:
            rb = PnPRansac(ex, problems)
        finally:
            os.environ.pop("ORBX_PNP", None)
        try:
            ps.assert_batch_equals_model(rb, problems, f"{what}, ORBX_PNP={env}")
            if replay:
                ps.assert_replay_equals_model(rb, problems, None, what)
        finally:
            rb.close()


def test_size_list_device_equals_host_path_equals_model(ex):
    probs = list(ps.size_problems())
    assert set(ps.GPU_N) <= {len(p["p3dw"]) for p in probs} and set(ps.GPU_ITERATIONS) <= {p["iterations"] for p in probs}
    assert {ps.HYP_LANES - 1, ps.HYP_LANES, ps.HYP_LANES + 1} <= {p["iterations"] for p in probs}
    check(ex, probs, "sizes")
    for p in probs[-3:]:                                        # the workgroup boundary of k_pnp_hypotheses, each alone
        check(ex, [p], f"hypothesis partition {p['iterations']}", replay=False)


def test_lds_chunk_boundaries(ex):
    check(ex, list(ps.chunk_problems()), "LDS chunks")


def test_mixed_call_with_problems_that_launch_nothing_and_no_problem_at_all(ex):
    mixed = ps.mixed_call()
    assert sum(not ps.launches(p) for p in mixed) == 2
    check(ex, mixed, "mixed")
    check(ex, [mixed[1], mixed[3]], "nothing launches")
    rb = PnPRansac(ex, [])
    assert len(rb) == 0
    rb.close()
    for k, p in enumerate(mixed):                              # a problem alone gives what it gives inside the batch
        check(ex, [p], f"single {k}", replay=False)


def test_planted_scenes_with_the_planar_and_the_identity_scene(ex):
    probs = list(ps.planted_scenes())
    assert any(p.get("plane") for p in probs) and any(np.array_equal(p["truth"], np.eye(4)) for p in probs)
    check(ex, probs, "planted")


def test_append_after_a_device_batch_gives_the_longer_batch(ex):
    """-2, then orbx_pnp_batch_append (host path) on a batch the device computed = the batch created with the longer set list"""
    p = ps.planted_scenes()[1]
    short = ps.variant(p, sets=p["sets"][:7], iterations=7)
    rb = PnPRansac(ex, [short])
    try:
        rb.append(0, p["sets"][7:])
        ps.assert_batch_equals_model(rb, [ps.variant(p, iterations=7)], "appended")
    finally:
        rb.close()


def test_outside_the_contract_equals_the_model(ex):
    probs = list(ps.poisoned())
    assert len(probs) == 8
    check(ex, probs, "outside the contract")
