"""Optimizer::OptimizeSim3 (orbx_optimize_sim3_batch), the part that needs no GPU: the library's host path through the C ABI on a
host-only handle against tests/sim3opt_model.py, bit for bit on the Sim3 doubles, the T12 floats, the keep bytes and the counts;
synthetic scenes with a known Sim3; every branch of the control asserted from the model's trace on committed seeds; the size
list; fix_scale; batches; the candidate loop with one batched call per round; inputs outside the contract; validation before
any work; the exp primitive against libm; the kernel's resources in the code object; the HIP-free unit under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/san_sim3opt.cpp, a stand-alone program).

The contract is device = host path = model.  Parity with a g2o + Eigen build is not pinned."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sim3opt_cases as cases
import sim3opt_model as sm
import sim3opt_scenes as ss
from orb_slam2_detailed_comments_amd import ORBextractor, OrbxError, _capi, optimizer, sim3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(built_lib):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    yield ex
    ex.close()


# ----------------------------------------------------------------------------------------------- sizes
def test_size_list_host_path_equals_model(host):
    scenes, models = cases.size_scenes()
    assert [s["n"] for s in scenes[::2]] == list(cases.SIZES) and {s["fix_scale"] for s in scenes} == {0, 1}
    cases.assert_all(cases.run(host, scenes), scenes, models, "sizes")
    for s, (res, keep) in zip(scenes, models):
        assert res["written"] == (1 if s["n"] >= 10 else 0), s["n"]      # no planted outliers below 19: 10 and 11 go on
        if s["n"] == 0:
            assert res["ninliers"] == 0 and res["ncorr"] == 0


# ----------------------------------------------------------------------------------------------- scenes with a known Sim3
TRUTH_SEEDS = ((1, 60, 0), (2, 60, 1), (3, 150, 0), (4, 25, 1))


def _truth_error(res, s):
    R = np.asarray(res["T12"], np.float64).reshape(4, 4)[:3, :3]
    return max(np.abs(R - s["s_true"] * s["R_true"]).max(), np.abs(np.asarray(res["t"]) - s["t_true"]).max(),
               abs(float(res["s"]) - s["s_true"]))


def test_noise_free_observations_give_the_true_sim3(host):
    """A convergence check, not a parity check.  The model's largest error on these seeds (max over |sR - sR_true|, |t - t_true|,
    |s - s_true|; the inputs are float32, the observations rounded to float32 pixels) measured on the CPU is 1.35e-7; the bound is
    ten times that."""
    scenes = [ss.make(seed, n, fs) for seed, n, fs in TRUTH_SEEDS]
    models = [cases.model(s) for s in scenes]
    got = cases.run(host, scenes)
    cases.assert_all(got, scenes, models, "noise-free")
    worst = 0.0
    for s, (res, keep), r in zip(scenes, models, got[0]):
        start = max(np.abs(np.float64(s["s"]) * s["R"].astype(np.float64) - s["s_true"] * s["R_true"]).max(),
                    np.abs(s["t"] - s["t_true"]).max())
        assert start > 5e-3                                              # the start is off by centimetres / degrees
        assert res["written"] == 1 and res["ninliers"] == s["n"] and keep.all()
        worst = max(worst, _truth_error(res, s))
        assert _truth_error(r, s) <= 1.35e-6
    print("largest error of the model against the true Sim3:", worst)
    assert worst <= 1.35e-6


def test_noise_and_planted_outliers(host):
    s = ss.make(5, 150, 0, noise=1.0, outlier_frac=0.2)
    want = cases.model(s)
    cases.assert_all(cases.run(host, [s]), [s], [want], "noisy")
    assert s["planted"].sum() >= 15 and not want[1][s["planted"]].any()  # every planted outlier (15 px and more) is nulled
    assert want[0]["written"] == 1 and want[0]["ninliers"] >= 100


# ----------------------------------------------------------------------------------------------- branches, from the trace
def test_every_branch_of_the_control_is_reached_and_agrees(host):
    scenes, models, traces = cases.branch_scenes()
    stages = [st for t in traces for st in t["stages"]]
    iters = [i for st in stages for i in st["iters"]]
    trials = [t for i in iters for t in i["trials"]]
    assert any(not t["early_return"] and t["nbad"] == 0 and t["more"] == 5 for t in traces)      # nBad == 0: 5 more
    assert any(not t["early_return"] and t["nbad"] > 0 and t["more"] == 10 for t in traces)      # nBad > 0: 10 more
    assert any(not t["accepted"] for t in trials)                               # a rejected trial (estimate restored)
    assert any(i["end"] == "trials" and len(i["trials"]) == 10 for i in iters)  # ten rejections: Terminate
    assert any(i["end"] == "rho0" for i in iters)                               # rho == 0
    assert any(i["end"] == "stall" for i in iters)                              # the three-stall ("Raul") stop
    early = [(s, m) for s, m, t in zip(scenes, models, traces) if t["early_return"] and t["nbad"] > 0]
    assert early                                                                # the early return 0 ...
    for s, (res, keep) in early:
        assert res["written"] == 0 and res["ninliers"] == 0
        assert np.count_nonzero(keep == 0) == res["nbad"] > 0                   # ... with the first test's nulls in keep
        inp = sm.result(sm.from_input(s["R"], s["t"], s["s"]), 0, 0, 0, 0)
        for f in ("r", "t", "s", "T12"):                                        # ... and r / t / s equal to the input
            assert np.asarray(res[f]).tobytes() == np.asarray(inp[f]).tobytes()
    branches = set().union(*[t.get("exp_branches", set()) for t in traces])
    assert branches == {"ss", "st", "Ss", "St"}                                 # all four eps branches of Sim3(Vector7d)
    cases.assert_all(cases.run(host, scenes), scenes, models, "branch seeds")


def test_fix_scale_keeps_column_six_zero_and_the_scale(host):
    scenes, models, traces = cases.branch_scenes()
    seen = 0
    for s, (res, keep), t in zip(scenes, models, traces):
        iters = [i for st in t["stages"] for i in st["iters"]]
        if s["fix_scale"]:
            seen += 1
            assert iters and all(i["col6_zero"] for i in iters)
            assert np.float64(res["s"]) == np.float64(s["s"])
            assert "Ss" not in t["exp_branches"] and "St" not in t["exp_branches"]
        else:
            assert not any(i["col6_zero"] for i in iters)
            assert res["written"] == 0 or np.float64(res["s"]) != np.float64(s["s"])
    assert seen >= 2
    got = cases.run(host, [s for s in scenes if s["fix_scale"]])
    assert all(np.float64(r["s"]) == np.float64(s["s"]) for r, s in zip(got[0], [s for s in scenes if s["fix_scale"]]))


# ----------------------------------------------------------------------------------------------- batches
def test_batch_of_16_mixed_problems_equals_16_single_calls(host):
    scenes, models, _ = cases.branch_scenes()
    sz, szm = cases.size_scenes()
    pick = [0, 3, 5, 6, 9, 10, 13, 14, 17, 20]
    sc = list(scenes) + [sz[k] for k in pick]
    mo = list(models) + [szm[k] for k in pick]
    assert len(sc) == 16
    whole = cases.run(host, sc)
    cases.assert_all(whole, sc, mo, "batch of 16")
    for k, s in enumerate(sc):
        one = cases.run(host, [s])
        assert one[0][0].tobytes() == whole[0][k].tobytes() and np.array_equal(one[1][0], whole[1][k]), k


class _FakeRansac:
    """solvers that return a Sim3 on chosen rounds: iterate(k, n) -> (T12 or None, no_more, inliers, ninliers)"""

    def __init__(self, extractor, plan):
        self.extractor, self.plan, self.round = extractor, plan, [0] * len(plan)

    def __len__(self):
        return len(self.plan)

    def iterate(self, k, n_iterations):
        r = self.round[k]
        self.round[k] += 1
        ret, no_more = self.plan[k][r] if r < len(self.plan[k]) else (False, True)    # past its plan: no more
        return (np.eye(4, dtype=np.float32) if ret else None), no_more, np.ones(4, bool), 4


def test_rounds_batched_accepts_what_the_round_robin_accepts(host):
    """solver 0 never returns and ends in round 2; solver 1 returns in round 1 a Sim3 whose optimisation keeps fewer than 20;
    solver 2 returns in round 2 (accepted); solver 3 returns in round 2 as well and would be accepted, but 2 comes first"""
    weak = ss.make(0, 14, 0, noise=1.0, outlier_frac=0.2)                  # returns 0
    good2 = ss.make(5, 150, 0, noise=1.0, outlier_frac=0.2)
    good3 = ss.make(3, 150, 0)
    plan = [[(False, False), (False, True)], [(True, False), (False, False)], [(False, False), (True, False)],
            [(False, False), (True, False)]]
    scene_of = {1: weak, 2: good2, 3: good3}
    accepted = {}

    def accept(k, T12, inliers, ninliers):
        res, keeps = optimizer.optimize_sim3_batch(host, [ss.problem(scene_of[k])])
        accepted["res"], accepted["keep"] = res[0].copy(), keeps[0]
        return res[0]["ninliers"] >= 20

    k_rr, calls_rr = sim3.compute_sim3_round_robin(_FakeRansac(host, plan), accept)
    k_b, calls_b, res_b, keep_b = sim3.compute_sim3_rounds_batched(_FakeRansac(host, plan), lambda k, T12, inl: ss.problem(scene_of[k]))
    assert k_rr == k_b == 2
    assert res_b.tobytes() == accepted["res"].tobytes() and np.array_equal(keep_b, accepted["keep"])
    assert calls_b[:len(calls_rr)] == calls_rr and calls_b[len(calls_rr):] == [(3, True, False, 4)]   # the one difference
    none = sim3.compute_sim3_rounds_batched(_FakeRansac(host, plan[:2]), lambda k, T12, inl: ss.problem(weak))
    assert none[0] == -1 and none[2] is None
    assert sim3.compute_sim3_rounds_batched(_FakeRansac(host, plan), lambda k, T12, inl: None)[0] == -1   # prepare gave nothing


# ----------------------------------------------------------------------------------------------- outside the contract
def test_outside_the_contract_ends_and_equals_the_model(host):
    spec = cases.special_scenes()
    scenes = [s for _, s in spec]
    traces = [{} for _ in scenes]
    models = [cases.model(s, t) for s, t in zip(scenes, traces)]
    got = cases.run(host, scenes)
    cases.assert_all(got, scenes, models, "outside the contract")
    by = {name: (m, t) for (name, _), m, t in zip(spec, models, traces)}
    for name, (m, t) in by.items():
        trials = [x for st in t["stages"] for i in st["iters"] for x in i["trials"]]
        assert trials, name
        if name in ("inf", "nan", "z = 0", "s = 0", "s = 0, fixed", "s = nan", "obs nan"):
            assert not any(x["accepted"] for x in trials), name          # nothing non-finite is accepted
    zi = [x for st in by["zero information"][1]["stages"] for i in st["iters"] for x in i["trials"]]
    assert zi and not any(x["ok"] for x in zi)                           # H = 0, lambda = 0: every solve fails, Terminate
    canon = 0
    for r in got[0]:
        for f in ("r", "t", "s", "T12"):
            a = np.atleast_1d(np.asarray(r[f]))
            nan = np.isnan(a)
            canon += int(nan.sum())
            assert (cases.bits(a[nan]) == (0x7ff8000000000000 if a.dtype == np.float64 else 0x7fc00000)).all()
    assert canon > 0                                                     # stored NaNs exist (s = nan) and are canonical


# ----------------------------------------------------------------------------------------------- validation
def test_validation_before_any_work(host):
    L, h = _capi.lib(), host.handle
    B, OK = _capi.BAD_ARGUMENT, _capi.OK
    s = ss.make(9, 12, 0, noise=1.0)
    probs = [ss.problem(s), ss.problem(s)]
    arr, hold, keeps = optimizer._sim3opt_marshal(probs)
    res = np.zeros(2, _capi.SIM3OPT_RESULT_DTYPE)
    res.view(np.uint8)[:] = 0xEE
    last = np.zeros((2, 8))

    def call(np_=2, pr=arr, rs=res):
        st = L.orbx_optimize_sim3_batch(h, np_, C.cast(pr, C.c_void_p) if pr is not None else None, _capi.ptr(rs))
        if st != OK:     # nothing is written on failure
            assert (res.view(np.uint8) == 0xEE).all() and all((k == ss.PREFILL_KEEP).all() for k in keeps)
        return st

    assert L.orbx_optimize_sim3_batch(None, 0, None, None) == B
    assert call(np_=-1) == B and call(pr=None) == B and call(rs=None) == B
    assert call(np_=0) == OK and call(np_=0, pr=None, rs=None) == OK and (res.view(np.uint8) == 0xEE).all()
    arr[1].n = -1; assert call() == B
    arr[1].n = 12
    for name in ("x1c", "x2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "keep"):
        was = getattr(arr[1], name)
        setattr(arr[1], name, None); assert call() == B, name
        setattr(arr[1], name, was)
    assert L.orbx_debug_sim3opt_inlier_test(h, 2, C.cast(arr, C.c_void_p), None, _capi.ptr(res)) == B
    assert L.orbx_debug_sim3opt_inlier_test(h, -1, C.cast(arr, C.c_void_p), _capi.ptr(last), _capi.ptr(res)) == B
    assert (res.view(np.uint8) == 0xEE).all()
    # n == 0 reads no array of the problem
    arr[0].n = 0
    for name in ("x1c", "x2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "keep"):
        setattr(arr[0], name, None)
    assert call() == OK
    assert res[0]["ninliers"] == 0 and res[0]["written"] == 0 and res[0]["ncorr"] == 0 and res[1]["ncorr"] == 12
    assert (keeps[0] == ss.PREFILL_KEEP).all() and (keeps[1][:12] != ss.PREFILL_KEEP).all()
    with pytest.raises(OrbxError) as e:                                  # the Python mirror raises what the C call returns
        _capi.check(L.orbx_optimize_sim3_batch(h, -1, None, None))
    assert e.value.status == B


# ----------------------------------------------------------------------------------------------- the inlier test alone
def test_inlier_test_reads_the_errors_of_the_last_trial(host):
    """orbx_debug_sim3opt_inlier_test runs the chi2 test of the host path with the Sim3 of the last trial given, a few
    centimetres and a percent of scale from the estimate: the flags are the model's at that Sim3 and differ from those at the
    estimate (asserted), so "test at the estimate" would fail here"""
    s, est8, last8 = cases.stale_case()
    cases.assert_inlier_test(cases.run_inlier_test(host, s, last8), s, est8, last8)


# ----------------------------------------------------------------------------------------------- the exp primitive
def test_exp_primitive_close_to_libm(built_lib):
    """largest relative difference from this machine's libm over the range a Sim3 update's sigma can take, [-3, 3], plus
    +-1e-9 (the numeric Jacobian's step) and 0; measured: 2.21e-16 = 0.994 x 2^-52"""
    L = _capi.lib()
    rng = np.random.default_rng(0)
    xs = np.concatenate([np.linspace(-3, 3, 20001), rng.uniform(-3, 3, 20000), [1e-9, -1e-9, 0.0]])
    worst = 0.0
    for x in xs:
        want = math.exp(x)
        worst = max(worst, abs(L.orbx_sim3opt_exp(float(x)) - want) / want)
    print("largest relative difference from libm:", worst)
    assert worst <= 2 ** -51
    assert L.orbx_sim3opt_exp(0.0) == 1.0
    assert L.orbx_sim3opt_exp(1e-9) == math.exp(1e-9) and L.orbx_sim3opt_exp(-1e-9) == math.exp(-1e-9)
    assert math.isnan(L.orbx_sim3opt_exp(float("nan")))
    assert L.orbx_sim3opt_exp(710.0) == math.inf and L.orbx_sim3opt_exp(float("inf")) == math.inf
    assert L.orbx_sim3opt_exp(-709.0) == 0.0 and L.orbx_sim3opt_exp(float("-inf")) == 0.0
    assert abs(L.orbx_sim3opt_exp(700.0) / math.exp(700.0) - 1) <= 2 ** -51 and abs(L.orbx_sim3opt_exp(-700.0) / math.exp(-700.0) - 1) <= 2 ** -51


# ----------------------------------------------------------------------------------------------- the kernel in the code object
def _header_enum(name):
    src = open(os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_sim3opt.h")).read()
    m = re.search(r"\b%s = (\d+)," % name, src)
    assert m, name
    return int(m.group(1))


def test_kernel_has_no_scratch_bounded_lds_and_calls_no_math_library(built_lib):
    from test_abi import _device_disassembly
    from test_pipeline_room import _kernel_metadata
    meta = _kernel_metadata(built_lib)
    hits = [v for k, v in meta.items() if "k_sim3_opt" in k]
    assert len(hits) == 1
    assert int(hits[0]["private_segment_fixed_size"]) == 0
    terms, nsim, sim = _header_enum("ORBX_SIM3OPT_TERMS"), _header_enum("ORBX_SIM3OPT_NSIM"), _header_enum("ORBX_SIM3OPT_SIM")
    assert (terms, nsim, sim) == (36, 15, 16)
    # the [36][65] term array plus the broadcast slots: the 36 sums and the table of the 15 Sim3 with their inverses
    assert int(hits[0]["group_segment_fixed_size"]) <= 8 * (terms * 65 + terms + nsim * sim)
    m = re.search(r"<_Z\d+k_sim3_opt[^>]*>:\n(.*?)s_endpgm", _device_disassembly(built_lib), re.S)
    assert m
    body = m.group(1)
    for op in ("v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64", "v_rsq_f64", "v_fma_f64"):
        assert op in body, op
    assert "v_sqrt_f64" not in body and "s_swappc" not in body and "v_sin" not in body and "v_cos" not in body and "v_exp" not in body


# ----------------------------------------------------------------------------------------------- sanitizers
def test_host_unit_clean_under_asan_ubsan(tmp_path):
    """csrc/orbx_sim3opt.cpp (validation, packing, the host path; HIP-free) built with g++ -fsanitize=address,undefined together
    with tests/san_sim3opt.cpp: the size list, every rejection, inputs outside the contract"""
    exe = str(tmp_path / "san_sim3opt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_sim3opt.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_sim3opt.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr
