"""Sim3Solver RANSAC on the device (orbx_sim3_ransac_batch_create: k_sim3_hypotheses, k_sim3_inliers) against the library's host
path (ORBX_SIM3=host on the same handle) and tests/sim3_model.py, on the scenes of the CPU tests.  Every comparison is exact:
hypothesis floats equal as uint32, masks, counts, every iterate return and the best state after every call.  Both fp_modes run
the same scenes and must give the same bits.  Sizes: N in {3, 20, 63, 64, 65, 129} (mask word boundaries and the tail) and
{512, 513, 1100} (the LDS chunk), iterations in {1, 5, 64, 65, 300} (wave and workgroup boundaries), problems of different N
and iteration counts mixed in one call with some that launch nothing, at most 16 problems per call, and no problem at all.
The model's answers are computed once per process (tests/sim3_scenes.py)."""
import os

import numpy as np
import pytest

import sim3_scenes as ss
from orb_slam2_detailed_comments_amd import ORBextractor, Sim3Ransac, _capi

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
    """device = model, then ORBX_SIM3=host on the same handle = model"""
    assert len(problems) <= 16
    for env in (None, "host"):
        if env:
            os.environ["ORBX_SIM3"] = env
        try:
            rb = Sim3Ransac(ex, problems)
        finally:
            os.environ.pop("ORBX_SIM3", None)
        try:
            ss.assert_batch_equals_model(rb, problems, f"{what}, ORBX_SIM3={env}")
            if replay:
                ss.assert_replay_equals_model(rb, problems, None, what)
        finally:
            rb.close()


def test_size_list_device_equals_host_path_equals_model(ex):
    probs = list(ss.size_problems())
    assert {len(p["x1c"]) for p in probs} == set(ss.GPU_N) and {p["iterations"] for p in probs} == set(ss.GPU_ITERATIONS)
    for a in range(0, len(probs), 16):
        check(ex, probs[a:a + 16], f"sizes {a}")


def test_lds_chunk_boundaries(ex):
    check(ex, list(ss.chunk_problems()), "LDS chunks")


def test_mixed_call_with_problems_that_launch_nothing_and_no_problem_at_all(ex):
    mixed = ss.mixed_call()
    assert sum(ss.model(p) is None for p in mixed) == 2
    check(ex, mixed, "mixed")
    check(ex, [mixed[1], mixed[3]], "nothing launches")
    rb = Sim3Ransac(ex, [])
    assert len(rb) == 0
    rb.close()
    for k, p in enumerate(mixed):                              # a problem alone gives what it gives inside the batch
        check(ex, [p], f"single {k}", replay=False)


def test_planted_scenes_and_the_control_edges(ex):
    check(ex, list(ss.planted_scenes()), "planted")
    base = ss.planted_scenes()[3]
    top = int(ss.model(base)[2].max())
    check(ex, [ss.variant(base, min_inliers=top), ss.make(21, 20, outlier_frac=0.0, min_inliers=20),
               ss.make(10, 30, iterations=1, min_inliers=6), ss.make(12, 100, iterations=300, min_inliers=20)], "control edges")


def test_outside_the_contract_equals_the_model(ex):
    probs = [ss.degenerate()]
    p = ss.make(43, 24, iterations=8, min_inliers=6)
    for poison in (np.inf, np.nan, 1e30, 0.0):
        x1 = p["x1c"].copy()
        x1[p["sets"][0, 0]] = poison
        x1[p["sets"][3, 1], 2] = poison
        probs.append(ss.variant(p, x1c=x1))
    a = ss.make(40, 50, iterations=20, min_inliers=10)
    probs += [a, ss.variant(a, fix_scale=1)]
    check(ex, probs, "outside the contract")
    hyps = ss.model(probs[0])[0]
    assert not np.isfinite(hyps[1][:12]).all()                 # the repeated index really is a non-finite hypothesis
