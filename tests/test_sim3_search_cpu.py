"""orbx_search_by_sim3_batch (ORBmatcher::SearchBySim3 batched, pose algebra included), the part that needs no GPU.  All
outputs are integers (and projections compared bit for bit), so every comparison is exact equality.

  * the planted items of tests/sim3_search_scenes.py hold on the model;
  * host path (through the C ABI, host-only handle) = tests/sim3_search_model.py on every scene, matches, count and every debug
    field, in both fp_modes;
  * the model's stage 1 fed to oracle.search_by_sim3 gives the same matches (an independent check of the selection);
  * the reference's compiled src/ORBmatcher.cc (oracle/_ref/libref_matcher_{strict,fma}.so), where it exists or can be built,
    gives the host path's matches and counts, scene by scene, problem by problem, and equals the records
    tests/golden/sim3_search_{strict,fma}.json (tools/sim3_search_record.py --record writes them; a test run never does); the host
    path reproduces the records whether or not the live library exists;
  * validation, one test per clause; compute_sim3_rounds_device against compute_sim3_rounds_batched; the HIP-free unit under
    AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program; no scratch in the kernels."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
import sim3_search_model as sm
import sim3_search_scenes as sc
import sim3opt_scenes as ss
from compat_scenes import target_dict
from orb_slam2_detailed_comments_amd import ORBextractor, ORBmatcher, OrbxError, _capi, sim3
from test_ref_matcher import entry, ref_harness, reference_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sim3_search_%s.json")
FIELDS = ("status1", "status2", "best1", "best2", "level1", "level2", "uv1", "uv2")
VARIANT = {_capi.FP_GCC_FMA: "fma", _capi.FP_STRICT: "strict"}


def thresholds(ex):
    thr = np.zeros(16, np.float32)
    _capi.check(_capi.lib().orbx_predict_scale_table(ex.handle, _capi.ptr(thr), 16))
    return thr


@pytest.fixture(scope="module", params=[_capi.FP_GCC_FMA, _capi.FP_STRICT], ids=["fma", "strict"])
def host(request, built_lib):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=-2, fp_mode=request.param)
    ex.fp = request.param
    ex.matcher = ORBmatcher(extractor=ex)
    yield ex
    ex.close()


_CACHE = {}


def scenes_and_models(ex):
    """the scenes and the model's results per fp_mode, computed once and shared"""
    thr = thresholds(ex)
    if "scenes" not in _CACHE:
        _CACHE["scenes"] = sc.all_scenes(thr)
    key = ("model", ex.fp)
    if key not in _CACHE:
        _CACHE[key] = {name: sm.search(s, ex.fp == _capi.FP_GCC_FMA, thr, sc.scale_table()) for name, s in _CACHE["scenes"].items()}
    return _CACHE["scenes"], _CACHE[key]


def assert_equals_model(got, model, what):
    counts, matches, dbg = got
    for k, m in enumerate(model):
        assert counts[k] == m["n"], (what, k, counts[k], m["n"])
        assert np.array_equal(matches[k], m["matches"]), (what, k)
        for f in FIELDS:
            np.testing.assert_array_equal(dbg[k][f], m[f], err_msg="%s problem %d %s" % (what, k, f))


def test_planted_items_hold_on_the_model_and_on_the_host_path(host):
    thr = thresholds(host)
    sc.planted_checks(thr)                                        # the generators produce every planted case (model alone)
    run = lambda s: host.matcher.SearchBySim3Batch(s["keyframes"], s["problems"], s["camera4"], s["bounds4"], debug=True)
    s, want = sc.planted_geometry()
    dbg = run(s)[2][0]
    for name, (i, st) in want.items():
        assert dbg["status1"][i] == st, (name, int(dbg["status1"][i]), st)
    s, want, mutual = sc.planted_selection()
    counts, matches, dbg = run(s)
    for name, (side, i, st, best) in want.items():
        assert dbg[0]["status%d" % side][i] == st and dbg[0]["best%d" % side][i] == best, name
    for name, (a, b) in mutual.items():
        assert matches[0][a] == b, name


def test_host_path_equals_the_model_on_every_scene(host):
    scenes, models = scenes_and_models(host)
    for name, s in scenes.items():
        got = host.matcher.SearchBySim3Batch(s["keyframes"], s["problems"], s["camera4"], s["bounds4"], debug=True)
        assert_equals_model(got, models[name], name)
        counts, matches = host.matcher.SearchBySim3Batch(s["keyframes"], s["problems"], s["camera4"], s["bounds4"])
        assert counts == got[0] and all(np.array_equal(a, b) for a, b in zip(matches, got[1]))
    assert sum(m["n"] for m in models["float"]) > 15 and sum(m["n"] for m in models["exact"]) > 15    # the scenes do match
    seen = set(np.concatenate([np.concatenate([m["status1"], m["status2"]]) for ms in models.values() for m in ms]).tolist())
    assert seen == set(range(7))


def test_model_stage_one_through_the_oracle_gives_the_host_paths_matches(host):
    scenes, models = scenes_and_models(host)
    thr = thresholds(host)
    got = {name: host.matcher.SearchBySim3Batch(s["keyframes"], s["problems"], s["camera4"], s["bounds4"]) for name, s in scenes.items()}
    for name, s in scenes.items():
        for k, p in enumerate(s["problems"]):
            k1, k2 = s["keyframes"][p["kf1"]], s["keyframes"][p["kf2"]]
            if len(k1["keys_un"]) == 0 or len(k2["keys_un"]) == 0:
                continue
            p12, p21, res = sm.stage1(s, host.fp == _capi.FP_GCC_FMA, thr, sc.scale_table(), k)
            n, m = oracle.search_by_sim3(target_dict(k1["keys_un"], k1["desc"]), target_dict(k2["keys_un"], k2["desc"]), p12, p21, p["th"])
            assert n == res["n"] and np.array_equal(m, res["matches"]), (name, k)
            assert n == got[name][0][k] and np.array_equal(m, got[name][1][k]), (name, k)   # ... and the host path's


def host_records(host):
    scenes, _ = scenes_and_models(host)
    out = {}
    for name, s in scenes.items():
        counts, matches = host.matcher.SearchBySim3Batch(s["keyframes"], s["problems"], s["camera4"], s["bounds4"])
        for k in range(len(counts)):
            out["%s/%d" % (name, k)] = dict(n=counts[k], matches=entry(matches[k]))
    return out


def test_host_path_reproduces_the_recorded_reference_outputs(host):
    with open(GOLDEN % VARIANT[host.fp]) as f:
        want = json.load(f)
    got = host_records(host)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


def test_compiled_reference_equals_the_host_path_and_the_records(host):
    if not reference_available():
        pytest.skip("neither oracle/_ref/ nor the reference tree is here: the recorded outputs stand in (the test above)")
    variant = VARIANT[host.fp]
    H = ref_harness(variant)
    scenes, _ = scenes_and_models(host)
    with open(GOLDEN % variant) as f:
        want = json.load(f)
    for name, s in scenes.items():
        counts, matches = host.matcher.SearchBySim3Batch(s["keyframes"], s["problems"], s["camera4"], s["bounds4"])
        for k, (n, m) in enumerate(sc.harness_search(H, s)):
            assert n == counts[k] and np.array_equal(m, matches[k]), (name, k, n, counts[k])
            assert want["%s/%d" % (name, k)] == dict(n=n, matches=entry(m)), (name, k)


# ----------------------------------------------------------------------------------------------- validation
class Call:
    """one valid two-keyframe, two-problem call through ctypes, whose pieces a test breaks one at a time"""

    def __init__(self, ex):
        s, _ = sc.planted_geometry()
        self.ex, self.keep = ex, []
        self.kfs = s["keyframes"]
        self.kv = (_capi.Sim3SearchKeyFrame * 2)()
        self.pv = (_capi.Sim3SearchProblem * 2)()
        self.n = [len(k["keys_un"]) for k in self.kfs]
        self.fill()
        self.out = [np.full(self.n[0], -1, np.int32) for _ in range(2)]
        self.rows = (C.c_void_p * 2)(*[o.ctypes.data for o in self.out])
        self.nf = (C.c_int * 2)()
        self.cam, self.bnd = sc.CAMERA4.copy(), sc.BOUNDS4.copy()

    def fill(self):
        for v, kf in zip(self.kv, self.kfs):
            arrs = [np.ascontiguousarray(kf[f]).copy() for f in ("keys_un", "desc", "has_point", "world_pos", "min_distance", "max_distance", "point_desc")]
            self.keep.append(arrs)
            v.n = len(arrs[0])
            v.Tcw[:] = np.eye(4, dtype=np.float32).reshape(16).tolist()
            v.keys_un, v.desc, v.has_point, v.world_pos, v.min_distance, v.max_distance, v.point_desc = [a.ctypes.data for a in arrs]
        for p in self.pv:
            p.kf1, p.kf2, p.s12, p.th = 0, 1, 1.0, 7.5
            p.R12[:] = np.eye(3, dtype=np.float32).reshape(9).tolist()
            p.matched1 = p.matched2 = None

    def __call__(self, nkf=2, nprob=2, h="own", kv="own", pv="own", cam="own", bnd="own", rows="own", nf="own"):
        own = lambda v, d: d if isinstance(v, str) else v
        return _capi.lib().orbx_search_by_sim3_batch(own(h, self.ex.handle), nkf, own(kv, C.cast(self.kv, C.c_void_p)), nprob,
                                                     own(pv, C.cast(self.pv, C.c_void_p)), own(cam, _capi.ptr(self.cam)),
                                                     own(bnd, _capi.ptr(self.bnd)), own(rows, C.cast(self.rows, C.c_void_p)),
                                                     own(nf, C.cast(self.nf, C.c_void_p)), None)


@pytest.fixture()
def call(host):
    c = Call(host)
    assert c() == _capi.OK
    return c


def test_negative_counts_are_bad_arguments(call):
    assert call(nkf=-1) == _capi.BAD_ARGUMENT and call(nprob=-1) == _capi.BAD_ARGUMENT
    call.kv[1].n = -1
    assert call() == _capi.BAD_ARGUMENT


def test_null_arguments_are_bad_arguments(call):
    for name in ("h", "kv", "pv", "cam", "bnd", "rows", "nf"):
        assert call(**{name: None}) == _capi.BAD_ARGUMENT, name
    call.rows[1] = None
    assert call() == _capi.BAD_ARGUMENT


@pytest.mark.parametrize("field", ["keys_un", "desc", "has_point", "world_pos", "min_distance", "max_distance", "point_desc"])
def test_a_null_field_of_a_non_empty_keyframe_is_a_bad_argument(call, field):
    setattr(call.kv[1], field, None)
    assert call() == _capi.BAD_ARGUMENT and b"null field" in _capi.lib().orbx_last_error()
    call.kv[1].n = 0                                              # an empty keyframe reads none of its arrays
    assert call() == _capi.OK


@pytest.mark.parametrize("which,bad", [("kf1", -1), ("kf1", 2), ("kf2", -1), ("kf2", 2)])
def test_an_index_outside_the_pool_is_a_bad_argument(call, which, bad):
    setattr(call.pv[1], which, bad)
    assert call() == _capi.BAD_ARGUMENT and b"pool" in _capi.lib().orbx_last_error()


@pytest.mark.parametrize("bad", [-1, 8])
def test_an_octave_outside_the_levels_is_a_bad_argument(call, bad):
    call.keep[1][0]["octave"][0] = bad
    assert call() == _capi.BAD_ARGUMENT and b"octave" in _capi.lib().orbx_last_error()


def test_bad_image_bounds_are_a_bad_argument(call):
    call.bnd[1] = call.bnd[0]
    assert call() == _capi.BAD_ARGUMENT


def test_more_than_65535_features_are_unsupported(call):
    call.kv[1].n = 65536                                          # refused before any array is read
    assert call() == _capi.UNSUPPORTED
    call.kv[1].n = call.n[1]
    assert call() == _capi.OK


def test_no_problem_launches_nothing_and_reads_nothing(call, host):
    assert call(nprob=0, pv=None, cam=None, bnd=None, rows=None, nf=None) == _capi.OK
    assert call(nkf=0, nprob=0, kv=None, pv=None, cam=None, bnd=None, rows=None, nf=None) == _capi.OK
    assert host.matcher.SearchBySim3Batch([], [], sc.CAMERA4, sc.BOUNDS4) == ([], [])
    with pytest.raises(OrbxError):
        host.matcher.SearchBySim3Batch([], [dict(kf1=0, kf2=0, s12=1.0, R12=np.eye(3), t12=np.zeros(3), th=7.5)], sc.CAMERA4, sc.BOUNDS4)


# ----------------------------------------------------------------------------------------------- the round driver
class _FakeRansac:
    def __init__(self, extractor, plan):
        self.extractor, self.plan, self.round = extractor, plan, [0] * len(plan)

    def __len__(self):
        return len(self.plan)

    def iterate(self, k, n_iterations):
        r = self.round[k]
        self.round[k] += 1
        ret, no_more = self.plan[k][r] if r < len(self.plan[k]) else (False, True)
        return (np.eye(4, dtype=np.float32) if ret else None), no_more, np.ones(4, bool), 4


def test_rounds_device_returns_what_rounds_batched_returns_with_the_single_search(host):
    """four solvers over the problems of the float scene; the optimisation problem of a solver is chosen by the number of
    matches its SearchBySim3 found, so a wrong search changes the accepted solver or its result"""
    scenes, models = scenes_and_models(host)
    s, thr = scenes["float"], thresholds(host)
    weak, good = ss.make(0, 14, 0, noise=1.0, outlier_frac=0.2), [ss.make(5, 150, 0, noise=1.0, outlier_frac=0.2), ss.make(3, 150, 0)]
    plan = [[(False, False), (False, True)], [(True, False), (False, False)], [(False, False), (True, False)],
            [(False, False), (True, False)]]
    seen = []

    def search(k, T12, inl):
        return s["problems"][k]

    def optimize(k, T12, inl, matches, nfound):
        seen.append((k, nfound, matches.tobytes()))
        return None if nfound == 0 else ss.problem(weak if k == 1 else good[nfound % 2])

    def prepare(k, T12, inl):                                     # the single SearchBySim3 on the model's projections
        p = s["problems"][k]
        k1, k2 = s["keyframes"][p["kf1"]], s["keyframes"][p["kf2"]]
        p12, p21, _ = sm.stage1(s, host.fp == _capi.FP_GCC_FMA, thr, sc.scale_table(), k)
        n, m = oracle.search_by_sim3(target_dict(k1["keys_un"], k1["desc"]), target_dict(k2["keys_un"], k2["desc"]), p12, p21, p["th"])
        return optimize(k, T12, inl, m, n)

    got = sim3.compute_sim3_rounds_device(_FakeRansac(host, plan), host.matcher, s["keyframes"], search, optimize, s["camera4"], s["bounds4"])
    mine, seen[:] = list(seen), []
    want = sim3.compute_sim3_rounds_batched(_FakeRansac(host, plan), prepare)
    assert mine == seen and len(mine) == 3 and all(n > 0 for _, n, _ in mine)
    assert got[0] == want[0] == 2 and got[1] == want[1]
    assert got[2].tobytes() == want[2].tobytes() and np.array_equal(got[3], want[3])
    none = sim3.compute_sim3_rounds_device(_FakeRansac(host, plan), host.matcher, s["keyframes"], lambda *a: None, optimize, s["camera4"], s["bounds4"])
    assert none[0] == -1 and none[2] is None


# ----------------------------------------------------------------------------------------------- the unit alone, the kernels
def test_host_unit_clean_under_asan_ubsan(tmp_path):
    """csrc/orbx_sim3search.cpp (validation, packing, the host path, the scatter; HIP-free) built with
    g++ -fsanitize=address,undefined together with tests/san_sim3search.cpp, a stand-alone program: sizes around 64, empty
    keyframes, the shared-KF1 batch, every validation failure"""
    exe = str(tmp_path / "san_sim3search")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "san_sim3search.cpp"),
                           os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "csrc", "orbx_sim3search.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "0 failures" in p.stdout and "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr


def test_kernels_have_no_scratch_and_no_lds(built_lib):
    from test_pipeline_room import _kernel_metadata
    meta = _kernel_metadata(built_lib)
    for name in ("k_sim3s_project", "k_sim3s_cand", "k_sim3s_mutual"):
        hits = [v for k, v in meta.items() if name in k]
        assert len(hits) == 1, name
        assert int(hits[0]["private_segment_fixed_size"]) == 0 and int(hits[0]["group_segment_fixed_size"]) == 0, name
        assert int(hits[0]["vgpr_count"]) <= 64, name                # 22 / 34 / 7 when this was written
