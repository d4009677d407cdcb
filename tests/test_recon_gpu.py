"""ReconstructH / ReconstructF on the device (orbx_init_reconstruct_batch_create: k_init_decompose, k_init_check_rt, k_init_pick)
against the library's host path (ORBX_RECON=host on the same handle) and tests/recon_model.py, on the scenes of the CPU tests, and
the fused call (orbx_initialize_batch_create, with k_init_select) against the two calls it replaces.  Every comparison is exact:
every R, t, n, cosine, parallax and point as uint32, every count, status byte, the chosen hypothesis and ok.  Both fp_modes run
the same scenes and must give the same bits.

Sizes: n in {1, 8, 63, 64, 65, 129} (one lane, the ballot word boundaries and the tail of k_init_check_rt's stride of 64) for H
(8 hypotheses) and F (4 hypotheses); every inlier count of the scene list, with the winner's nGood in {0, 1, 50, 51, 52, 80} on
both sides of idx = min(50, size - 1) of the selection; a mixed call of both models with different n and two problems that
launch nothing, no problem at all, and each problem alone.  At most 16 problems per call.  The model's answers are computed once
per process (tests/recon_scenes.py)."""
import os

import pytest

import init_scenes as isc
import recon_model as rm
import recon_scenes as sc
from orb_slam2_detailed_comments_amd import InitializerRansac, InitializerReconstruct, ORBextractor, _capi, initialize_batch

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
    """device = model, then ORBX_RECON=host on the same handle = model"""
    assert len(problems) <= 16
    for env in (None, "host"):
        if env:
            os.environ["ORBX_RECON"] = env
        try:
            rc = InitializerReconstruct(ex, problems)
        finally:
            os.environ.pop("ORBX_RECON", None)
        try:
            sc.assert_batch_equals_model(rc, problems, f"{what}, ORBX_RECON={env}")
        finally:
            rc.close()


def test_size_list_device_equals_host_path_equals_model(ex):
    probs = list(sc.size_problems())
    assert {len(p["matches"]) for p in probs} == set(sc.GPU_N) and {p["model"] for p in probs} == {rm.H, rm.FUND}
    check(ex, probs, "sizes")
    for p in probs[:4]:                                          # n = 1 and n = 8, each alone
        check(ex, [p], f"n = {len(p['matches'])} alone")


def test_every_case_of_the_scene_list(ex):
    c = sc.cases()
    names = list(c)
    assert {max(h["nGood"] for h in sc.model_of(c[f"winner_{k}"])["hyp"]) for k in sc.WINNER_COUNTS} == set(sc.WINNER_COUNTS)
    check(ex, [c[k] for k in names[:10]], "cases a")
    check(ex, [c[k] for k in names[10:]], "cases b")


def test_mixed_call_with_problems_that_launch_nothing_and_no_problem_at_all(ex):
    mixed = sc.mixed_call()
    assert len(mixed) <= 16 and sum(sc.model_of(p)["N"] == 0 for p in mixed) == 2
    check(ex, mixed, "mixed")
    check(ex, [mixed[1], mixed[4]], "nothing launches")
    rc = InitializerReconstruct(ex, [])
    assert len(rc) == 0
    rc.close()
    for k, p in enumerate(mixed):                              # a problem alone gives what it gives inside the batch
        check(ex, [p], f"single {k}")


def fused_equals_two_calls(ex, problems, what):
    cams = [sc.camera() for _ in problems]
    rb, rc = initialize_batch(ex, problems, cams)
    rb2 = InitializerRansac(ex, problems)
    try:
        isc.assert_batch_equals_model(rb, problems, f"{what}: RANSAC half")
        alone = [sc.from_ransac(p, rb2.result(k), cams[k]) for k, p in enumerate(problems)]
        sc.assert_batch_equals_model(rc, alone, f"{what}: reconstruction half")
        rc2 = InitializerReconstruct(ex, alone)
        try:
            for k, q in enumerate(alone):
                nh = 8 if q["model"] == rm.H else 4
                want = dict(rc2.result(k), hyp=[rc2.hypothesis(k, i) for i in range(nh)])
                sc.assert_result_equals(rc.result(k), [rc.hypothesis(k, i) for i in range(nh)], want, f"{what}: fused = two calls, problem {k}")
        finally:
            rc2.close()
        return [rb.result(k) for k in range(len(problems))], [rc.result(k) for k in range(len(problems))]
    finally:
        rb.close(), rc.close(), rb2.close()


def test_fused_call_equals_ransac_followed_by_the_stand_alone_call(ex):
    probs = sc.ransac_problems()
    ran, rec = fused_equals_two_calls(ex, probs, "fused")
    assert [r["model"] for r in ran][:5] == [rm.H, rm.FUND, rm.im.NONE, rm.H, rm.im.NONE]
    assert rec[1]["ok"] and not rec[2]["ok"] and not rec[4]["ok"] and rec[2]["N"] == 0 and rec[2]["chosen"] == -1
    assert not rec[3]["ok"]                                      # the pure rotation
    fused_equals_two_calls(ex, [probs[1]], "fused, one problem")
    fused_equals_two_calls(ex, [probs[2], probs[4]], "fused, nothing to reconstruct")
    rb, rc = initialize_batch(ex, [], [])
    assert len(rb) == 0 and len(rc) == 0
    rb.close(), rc.close()
