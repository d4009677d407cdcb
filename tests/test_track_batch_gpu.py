"""Batched device-resident SearchByProjection of the two tracking matchers on the GPU (k_track_project, k_track_cand,
k_track_select): every problem of every call equals, bit for bit, BOTH the C oracle and the existing single call fed that
frame's keypoints, descriptors and u_right -- in both fp_modes, on random conflict-heavy scenes (tests/track_model.py) and on
planted edges, each in a problem of its own.  tests/track_model.py also tells that the inputs do contain what they are meant to:
rescans, overrides, accept events in dropped bins.  Entries of an output row past the frame's count keep the sentinel."""
import types

import numpy as np
import pytest

import oracle
import track_model as tm
from orb_slam2_detailed_comments_amd import ORBextractor, ORBmatcher, _capi, synth

pytestmark = pytest.mark.gpu
CAP = 512
SENTINEL = -77
F32 = np.float32


# ----------------------------------------------------------------------------------------------- plumbing
class DeviceBatch:
    """frames (tests/track_model.py dicts) as the buffers a device batch leaves behind, `cap` records apart, plus their grids"""

    def __init__(self, ex, frames, cap=CAP, with_u_right=True, bounds=tm.BOUNDS):
        import torch
        self.torch, self.ex, self.frames, self.cap, self.bounds = torch, ex, frames, cap, bounds
        nf = len(frames)
        keys = np.zeros((nf, cap), _capi.KP_DTYPE); desc = np.zeros((nf, cap, 32), np.uint8)
        ur = np.full((nf, cap), -1.0, np.float32); cnt = np.zeros(nf, np.int32)
        for f, fr in enumerate(frames):
            n = len(fr["keys"])
            assert n <= cap
            keys[f, :n], desc[f, :n], ur[f, :n], cnt[f] = fr["keys"], fr["desc"], fr["u_right"], n
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(nf, -1) if a.dtype == _capi.KP_DTYPE else a).to(dev)
        self.keys, self.desc, self.cnt = up(keys), up(desc), up(cnt)
        self.ur = up(ur) if with_u_right else None
        self.cb = torch.zeros((nf, 64 * 48 + 1), dtype=torch.int32, device=dev)
        self.it = torch.zeros((nf, cap), dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        b4 = np.asarray(bounds, np.float32)
        _capi.check(_capi.lib().orbx_grid_build_device(ex.handle, nf, _capi.ptr(self.keys), _capi.ptr(self.cnt), cap, _capi.ptr(b4),
                                                       _capi.ptr(self.cb), _capi.ptr(self.it)))
        ex.synchronize()

    def args(self):
        return dict(nframes=len(self.frames), keys_un=self.keys, desc=self.desc, u_right=self.ur, counts=self.cnt, cap=self.cap,
                    cell_begin=self.cb, items=self.it, bounds=self.bounds)

    def outputs(self, k):
        torch = self.torch
        dev = torch.device("cuda", 0)
        rows = torch.full((max(k, 1), self.cap), SENTINEL, dtype=torch.int32, device=dev)
        nm = torch.full((max(k, 1),), SENTINEL, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        return rows, nm


def _view(fr):
    """what the single calls read of a frame.Frame"""
    return types.SimpleNamespace(mvKeysUn=np.ascontiguousarray(fr["keys"], _capi.KP_DTYPE), mDescriptors=np.ascontiguousarray(fr["desc"]),
                                 mvuRight=np.ascontiguousarray(fr["u_right"], np.float32), N=len(fr["keys"]), bounds=tm.BOUNDS)


def run_ff(ex, batch, probs, ori):
    m = ORBmatcher(0.8, ori, extractor=ex)
    rows, nm = batch.outputs(len(probs))
    m.SearchByProjectionBatchDevice(probs, batch.args(), K=tm.CAMERA, mb=tm.MB, mbf=tm.MBF, d_matched_last=rows, d_nmatches=nm)
    ex.synchronize()
    return nm.cpu().numpy(), rows.cpu().numpy()


def run_mp(ex, batch, probs, ratio):
    m = ORBmatcher(ratio, True, extractor=ex)
    rows, nm = batch.outputs(len(probs))
    m.SearchByProjectionMapPointsBatchDevice(probs, batch.args(), d_assigned=rows, d_nmatches=nm)
    ex.synchronize()
    return nm.cpu().numpy(), rows.cpu().numpy()


def single_ff(ex, fr, p, ori):
    m = ORBmatcher(0.8, ori, extractor=ex)
    last = types.SimpleNamespace(mvKeysUn=np.ascontiguousarray(p["keys_un"], _capi.KP_DTYPE), N=len(p["keys_un"]))
    return m.SearchByProjection(_view(fr), last, float(p["th"]), p["mono"], Tcw=p["Tcw"], Tlw=p["Tlw"], K=tm.CAMERA, mb=tm.MB,
                                mbf=tm.MBF, has_map_point=p["has_map_point"], world_pos=p["world_pos"], mp_desc=p["mp_desc"],
                                observations=p["observations"])


def single_mp(ex, fr, p, ratio):
    m = ORBmatcher(ratio, True, extractor=ex)
    n = len(fr["keys"])
    fo = p["frame_observations"]
    fo = np.full(n, -1, np.int32) if fo is None else fo[:n]
    return m.SearchByProjectionMapPoints(_view(fr), float(p["th"]), frame_observations=fo, in_view=p["in_view"], proj=p["proj"],
                                         level=p["level"], view_cos=p["view_cos"], mp_desc=p["mp_desc"], observations=p["observations"])


def check_ff(ex, fp, batch, probs, ori, scale, tag=""):
    nm, rows = run_ff(ex, batch, probs, ori)
    for k, p in enumerate(probs):
        fr = batch.frames[p["frame"]]
        n = len(fr["keys"])
        on, om = tm.oracle_ff(fr, p, ori, fp, scale)
        sn, sm = single_ff(ex, fr, p, ori)
        print(f"{tag} ff problem {k}: frame {p['frame']} n {n} points {len(p['keys_un'])} nmatches {nm[k]} oracle {on} single {sn}")
        assert nm[k] == sn and np.array_equal(rows[k, :n], sm), f"{tag} problem {k} differs from the single call"
        assert nm[k] == on and np.array_equal(rows[k, :n], om), f"{tag} problem {k} differs from the oracle"
        assert (rows[k, n:] == SENTINEL).all(), f"{tag} problem {k}: entries past the frame's count were written"
    return nm, rows


def check_mp(ex, batch, probs, ratio, scale, tag=""):
    nm, rows = run_mp(ex, batch, probs, ratio)
    for k, p in enumerate(probs):
        fr = batch.frames[p["frame"]]
        n = len(fr["keys"])
        po = p if p["frame_observations"] is not None else dict(p, frame_observations=np.full(max(n, 1), -1, np.int32))
        on, oa = tm.oracle_mp(fr, po, ratio, scale)
        sn, sa = single_mp(ex, fr, p, ratio)
        print(f"{tag} mp problem {k}: frame {p['frame']} n {n} points {len(p['in_view'])} nmatches {nm[k]} oracle {on} single {sn}")
        assert nm[k] == sn and np.array_equal(rows[k, :n], sa), f"{tag} problem {k} differs from the single call"
        assert nm[k] == on and np.array_equal(rows[k, :n], oa), f"{tag} problem {k} differs from the oracle"
        assert (rows[k, n:] == SENTINEL).all(), f"{tag} problem {k}: entries past the frame's count were written"
    return nm, rows


@pytest.fixture(scope="module", params=[_capi.FP_GCC_FMA, _capi.FP_STRICT], ids=["fma", "strict"])
def exfp(request):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, fp_mode=request.param)
    scale = tm.scale_factors()
    assert np.array_equal(ex.GetScaleFactors()[:8], scale)
    yield ex, request.param, scale
    ex.close()


@pytest.fixture(scope="module")
def random_frames():
    rng = np.random.default_rng(77)
    return [tm.make_frame(rng, n) for n in (300, 150, 37, 1)]


# ----------------------------------------------------------------------------------------------- the main sweep
def test_frame_policy_sweep(exfp, random_frames):
    ex, fp, scale = exfp
    batch = DeviceBatch(ex, random_frames)
    rng = np.random.default_rng(101)
    probs = []
    for k in range(9):   # mono / stereo x forward / backward / sideways x th 7 / 15 / 30
        f = (0, 0, 1, 1, 2, 0, 1, 3, 0)[k]
        probs.append(dict(tm.make_ff_problem(rng, random_frames[f], int(rng.integers(100, 400)),
                                             motion=("forward", "backward", "side")[k % 3], th=(7.0, 15.0, 30.0)[(k // 3) % 3],
                                             mono=int(k in (2, 4, 6)), scale=scale), frame=f))
    total = 0
    for ori in (True, False):
        nm, _ = check_ff(ex, fp, batch, probs, ori, scale, f"sweep ori={ori}")
        total += int(nm.sum())
    assert total > 500
    if fp == _capi.FP_STRICT:   # the model restates the strict arithmetic: the sweep holds rescans, overrides, dropped events
        tot = dict(rescans=0, overrides=0, dropped_events=0, kept_overridden=0)
        for p in probs:
            st = tm.model_ff(random_frames[p["frame"]], p, True, scale)[2]
            for key in tot:
                tot[key] += st[key]
        print("frame policy sweep:", tot)
        assert all(v > 0 for v in tot.values()), tot


def test_mappoint_policy_sweep(exfp, random_frames):
    ex, fp, scale = exfp
    batch = DeviceBatch(ex, random_frames)
    rng = np.random.default_rng(202)
    probs = []
    for k in range(9):
        f = (0, 1, 0, 2, 1, 0, 3, 0, 1)[k]
        probs.append(dict(tm.make_mp_problem(rng, random_frames[f], int(rng.integers(100, 400)), th=(1.0, 3.0, 5.0)[k % 3], cap=CAP),
                          frame=f))
    probs[4]["frame_observations"] = None
    total, tot = 0, dict(rescans=0, ratio_rejects=0)
    for ratio in (0.6, 0.8, 1.0):
        nm, _ = check_mp(ex, batch, probs, ratio, scale, f"sweep ratio={ratio}")
        total += int(nm.sum())
        for p in probs:
            po = p if p["frame_observations"] is not None else dict(p, frame_observations=np.full(CAP, -1, np.int32))
            st = tm.model_mp(random_frames[p["frame"]], po, ratio, scale)[2]
            for key in tot:
                tot[key] += st[key]
    print("map-point policy sweep:", tot)
    assert total > 500 and all(v > 0 for v in tot.values()), (total, tot)


def test_without_u_right_every_feature_is_monocular(exfp, random_frames):
    ex, fp, scale = exfp
    mono_frames = [dict(fr, u_right=np.full(len(fr["keys"]), -1.0, np.float32)) for fr in random_frames]
    batch = DeviceBatch(ex, mono_frames, with_u_right=False)
    rng = np.random.default_rng(303)
    fprobs = [dict(tm.make_ff_problem(rng, mono_frames[f], 200, motion="side", th=15.0, mono=1, scale=scale), frame=f) for f in (0, 1)]
    mprobs = [dict(tm.make_mp_problem(rng, mono_frames[f], 200, cap=CAP), frame=f) for f in (0, 1)]
    assert check_ff(ex, fp, batch, fprobs, True, scale, "no u_right")[0].sum() > 50
    assert check_mp(ex, batch, mprobs, 0.8, scale, "no u_right")[0].sum() > 50


def test_upstream_pyramid_mode_handle(random_frames):
    """the matchers read no pyramid; a handle in the other pyramid mode gives the same results"""
    ex = ORBextractor(1000, 1.2, 8, 20, 7, pyramid_mode=_capi.PYRAMID_UPSTREAM)
    scale = tm.scale_factors()
    batch = DeviceBatch(ex, random_frames)
    rng = np.random.default_rng(404)
    fprobs = [dict(tm.make_ff_problem(rng, random_frames[0], 300, motion="forward", th=15.0, scale=scale), frame=0)]
    mprobs = [dict(tm.make_mp_problem(rng, random_frames[1], 300, cap=CAP), frame=1)]
    assert check_ff(ex, _capi.FP_GCC_FMA, batch, fprobs, True, scale, "upstream")[0].sum() > 20
    assert check_mp(ex, batch, mprobs, 0.8, scale, "upstream")[0].sum() > 20
    ex.close()


# ----------------------------------------------------------------------------------------------- planted edges
def bits(d, start=0):
    """a descriptor with d bits set from bit `start` on: distance d to the zero descriptor"""
    out = np.zeros(32, np.uint8)
    for b in range(start, start + d):
        out[(b % 256) >> 3] |= np.uint8(1 << (b & 7))
    return out


def planted_frame(feats):
    """feats: (x, y, octave, descriptor, u_right, angle)"""
    n = len(feats)
    k = np.zeros(n, oracle.KP_DTYPE)
    d = np.zeros((n, 32), np.uint8)
    ur = np.full(n, -1.0, np.float32)
    for i, (x, y, o, de, u, a) in enumerate(feats):
        k["x"][i], k["y"][i], k["octave"][i], k["angle"][i] = x, y, o, a
        d[i], ur[i] = de, u
    return dict(keys=k, desc=d, u_right=ur, depth=np.ones(n))


def planted_ff(points, th=7.0, mono=1, motion="side"):
    """points: (u, v, octave, descriptor, observations, angle, has_map_point, z).  Identity pose: the point projects to (u, v)
    (u exactly where u - 100 is a multiple of 15 and z = 1), ur = u - 40 / z; tlc = (0, 0, +-0.5 | 0)"""
    fx, fy, cx, cy = tm.CAMERA
    n = len(points)
    kl = np.zeros(n, oracle.KP_DTYPE)
    xw = np.zeros((n, 3), np.float32); de = np.zeros((n, 32), np.uint8)
    has = np.zeros(n, np.uint8); obs = np.zeros(n, np.int32)
    for i, (u, v, o, d, ob, a, h, z) in enumerate(points):
        kl["octave"][i], kl["angle"][i] = o, a
        xw[i] = (F32((u - cx) / fx * z), F32((v - cy) / fy * z), F32(z))
        de[i], has[i], obs[i] = d, h, ob
    Tlw = np.eye(4, dtype=np.float32)
    Tlw[2, 3] = {"forward": 0.5, "backward": -0.5, "side": 0.0}[motion]
    return dict(th=F32(th), mono=mono, Tcw=np.eye(4, dtype=np.float32), Tlw=Tlw, keys_un=kl, has_map_point=has, world_pos=xw,
                mp_desc=de, observations=obs)


def planted_mp(points, th=3.0, frame_observations=None):
    """points: (x, y, xr, level, descriptor, observations, in_view, view_cos)"""
    n = len(points)
    proj = np.zeros((n, 3), np.float32); de = np.zeros((n, 32), np.uint8)
    lvl = np.zeros(n, np.int32); obs = np.zeros(n, np.int32); iv = np.zeros(n, np.uint8); vc = np.zeros(n, np.float32)
    for i, (x, y, xr, l, d, ob, v, c) in enumerate(points):
        proj[i], lvl[i], de[i], obs[i], iv[i], vc[i] = (x, y, xr), l, d, ob, v, c
    return dict(th=F32(th), frame_observations=frame_observations, in_view=iv, proj=proj, level=lvl, view_cos=vc, mp_desc=de,
                observations=obs)


Z = bits(0)


def lattice(nbins_counts, override_rot=None):
    """isolated (feature, point) pairs 12 px apart, distance 0 each, th 7 on octave 0: everyone matches its own feature; the
    rotation of pair i is 12 degrees x its bin: counts = {bin: events}"""
    feats, pts = [], []
    i = 0
    for b, c in nbins_counts.items():
        for _ in range(c):
            x, y = 10.0 + 12.0 * (i % 15), 10.0 + 12.0 * (i // 15)
            de = bits(3, 8 * (i % 30))
            feats.append((x, y, 0, de, -1.0, 0.0))
            pts.append((x, y, 0, de, 1, 12.0 * b, 1, 1.0))
            i += 1
    return feats, pts


def planted_ff_cases():
    """[(name, frame, problem, expect(nm, row, stats))] -- one problem each"""
    cases = []
    # a bucket of 70 features: one cell (3.125 px wide), exact ties inside it -- the first visited (lowest index) wins
    feats = [(50.0 + 0.01 * i, 50.0, 0, bits(20 if i not in (3, 66) else 1, i), -1.0, 0.0) for i in range(70)]
    cases.append(("bucket>64", planted_frame(feats), planted_ff([(50.0, 50.0, 0, Z, 1, 0.0, 1, 1.0)]),
                  lambda nm, row, st: nm == 1 and row[3] == 0 and row[66] == -1))
    # a window over several cell columns that hangs over the grid edge (r = 30 * 1.44 around (2, 3))
    feats = [(1.0 + 4.0 * i, 2.0 + 3.0 * (i % 5), 2, bits(2 + i), -1.0, 0.0) for i in range(12)]
    cases.append(("over-the-edge", planted_frame(feats), planted_ff([(2.0, 3.0, 2, Z, 1, 0.0, 1, 1.0)], th=30.0),
                  lambda nm, row, st: nm == 1 and row[0] == 0))
    # a projection outside the bounds and a point behind the camera take no part; the third point does
    feats = [(100.0, 75.0, 0, bits(1), -1.0, 0.0), (130.0, 75.0, 0, bits(2), -1.0, 0.0)]
    cases.append(("outside-bounds", planted_frame(feats),
                  planted_ff([(250.0, 75.0, 0, Z, 1, 0.0, 1, 1.0), (130.0, 75.0, 0, Z, 1, 0.0, 1, 1.0)]),
                  lambda nm, row, st: nm == 1 and row[0] == -1 and row[1] == 1))
    cases.append(("negative-invz", planted_frame(feats),
                  planted_ff([(100.0, 75.0, 0, Z, 1, 0.0, 1, -1.0), (130.0, 75.0, 0, Z, 1, 0.0, 1, 1.0)]),
                  lambda nm, row, st: nm == 1 and row[0] == -1 and row[1] == 1))
    # octave 0 under forward motion: GetFeaturesInArea(minLevel = 0, maxLevel = -1) checks no level at all
    feats = [(100.0, 75.0, 5, bits(1), -1.0, 0.0), (101.0, 75.0, 0, bits(9), -1.0, 0.0)]
    cases.append(("octave0-forward", planted_frame(feats), planted_ff([(100.0, 75.0, 0, Z, 1, 0.0, 1, 1.0)], mono=0, motion="forward"),
                  lambda nm, row, st: nm == 1 and row[0] == 0))
    # ... while octave 1 forward keeps octaves >= 1 and backward keeps octaves <= 1
    feats = [(100.0, 75.0, 0, bits(1), -1.0, 0.0), (101.0, 75.0, 3, bits(9), -1.0, 0.0)]
    cases.append(("octave1-forward", planted_frame(feats), planted_ff([(100.0, 75.0, 1, Z, 1, 0.0, 1, 1.0)], mono=0, motion="forward"),
                  lambda nm, row, st: nm == 1 and row[1] == 0))
    cases.append(("octave1-backward", planted_frame(feats), planted_ff([(100.0, 75.0, 1, Z, 1, 0.0, 1, 1.0)], mono=0, motion="backward"),
                  lambda nm, row, st: nm == 1 and row[0] == 0))
    # an exact tie across buckets: the lower cell column is visited first, whatever the feature index
    feats = [(60.0, 50.0, 0, bits(5, 0), -1.0, 0.0), (52.0, 50.0, 0, bits(5, 40), -1.0, 0.0)]
    cases.append(("tie-across-buckets", planted_frame(feats), planted_ff([(56.0, 50.0, 0, Z, 1, 0.0, 1, 1.0)], th=7.0),
                  lambda nm, row, st: nm == 1 and row[1] == 0 and row[0] == -1))
    # two observed points want the same feature: the second one walks its window again and takes the next best
    feats = [(100.0, 75.0, 0, bits(2), -1.0, 0.0), (102.0, 75.0, 0, bits(10), -1.0, 0.0)]
    cases.append(("blocked-rescan", planted_frame(feats),
                  planted_ff([(100.0, 75.0, 0, Z, 2, 0.0, 1, 1.0), (101.0, 75.0, 0, Z, 2, 0.0, 1, 1.0)]),
                  lambda nm, row, st: nm == 2 and row[0] == 0 and row[1] == 1 and st["rescans"] == 1))
    # a 0-observation point (a temporal stereo point) is overridden by a later one.  Its own accept event lands in a dropped
    # bin: the feature loses its match although the later, kept event owned it.  20 pairs in bin 0 make bin 8 droppable.
    for name, rot0, expect in (("override-dropped", 96.0, lambda nm, row, st: nm == 21 and row[20] == -1 and st["overrides"] == 1
                                and st["dropped_events"] == 1 and st["kept_overridden"] == 1),
                               ("override-kept", 0.0, lambda nm, row, st: nm == 22 and row[20] == 21 and st["overrides"] == 1
                                and st["dropped_events"] == 0)):
        feats, pts = lattice({0: 20})
        feats.append((100.0, 140.0, 0, bits(2), -1.0, 0.0))
        pts.append((100.0, 140.0, 0, Z, 0, rot0, 1, 1.0))         # Observations() == 0: does not block feature 20
        pts.append((101.0, 140.0, 0, Z, 1, 0.0, 1, 1.0))
        cases.append((name, planted_frame(feats), planted_ff(pts), expect))
    # u_right exactly at the radius passes (`> radius` rejects); one ulp further does not
    u, r = 130.0, 15.0                                              # exact: (130 - 100) / 120 = 0.25; ur = 130 - 40 = 90
    for name, off, want in (("u_right-at-radius", F32(90.0 + r), 0), ("u_right-past-radius", np.nextafter(F32(90.0 + r), F32(1e9)), 1)):
        feats = [(130.0, 75.0, 0, bits(1), off, 0.0), (131.0, 75.0, 0, bits(30), F32(91.0), 0.0)]
        cases.append((name, planted_frame(feats), planted_ff([(u, 75.0, 0, Z, 1, 0.0, 1, 1.0)], th=15.0, mono=0),
                      lambda nm, row, st, want=want: nm == 1 and row[want] == 0 and row[1 - want] == -1))
    # histograms: one bin; a second / third bin below a tenth of the first is dropped
    for name, counts, nm_want in (("one-bin", {4: 25}, 25), ("second-dropped", {0: 30, 5: 2, 9: 1}, 30),
                                  ("third-dropped", {0: 30, 5: 5, 9: 2}, 35), ("three-kept", {0: 30, 5: 5, 9: 3, 12: 1}, 38)):
        feats, pts = lattice(counts)
        cases.append((name, planted_frame(feats), planted_ff(pts),
                      lambda nm, row, st, w=nm_want, tot=sum(counts.values()): nm == w and st["dropped_events"] == tot - w))
    # degenerate problems
    feats, pts = lattice({0: 10})
    cases.append(("count-0", planted_frame([]), planted_ff(pts), lambda nm, row, st: nm == 0))
    cases.append(("view-n-0", planted_frame(feats), planted_ff([]), lambda nm, row, st: nm == 0 and (row == -1).all()))
    none = planted_ff(pts); none["has_map_point"][:] = 0
    cases.append(("no-map-points", planted_frame(feats), none, lambda nm, row, st: nm == 0 and (row == -1).all()))
    return cases


def test_frame_policy_planted_edges(exfp):
    ex, fp, scale = exfp
    cases = planted_ff_cases()
    rng = np.random.default_rng(9)
    full = tm.make_frame(rng, CAP)                                  # a frame whose count equals cap
    cases.append(("count==cap", full, tm.make_ff_problem(rng, full, 300, motion="side", th=15.0, scale=scale),
                  lambda nm, row, st: nm > 50 and st["rescans"] > 0))
    frames = [c[1] for c in cases]
    probs = [dict(c[2], frame=i) for i, c in enumerate(cases)]
    probs.append(dict(probs[-1], th=F32(30.0)))                     # the same frame in two problems: the retry with 2 * th
    batch = DeviceBatch(ex, frames)
    nm, rows = check_ff(ex, fp, batch, probs, True, scale, "planted")
    for i, (name, fr, p, expect) in enumerate(cases):
        st = tm.model_ff(fr, p, True, scale)[2]
        assert expect(int(nm[i]), rows[i, :len(fr["keys"])], st), (name, int(nm[i]), st, rows[i, :len(fr["keys"])][:30])
    assert nm[-1] > 50 and not np.array_equal(rows[-1], rows[-2])
    check_ff(ex, fp, batch, probs, False, scale, "planted, no orientation check")


def planted_mp_cases():
    cases = []
    V = 0.99   # view_cos: r = 4 * th * scale[level]; th 3 on level 0 -> 12
    # best and second on the same level, the ratio exactly on the boundary (8 > 0.8f * 10 is false in float): accepted
    for name, d1, d2, o2, want in (("ratio-boundary-same-level", 8, 10, 1, 1), ("ratio-fails-same-level", 9, 10, 1, 0),
                                   ("ratio-different-levels", 9, 10, 0, 1)):
        feats = [(100.0, 75.0, 1, bits(d1), -1.0, 0.0), (103.0, 75.0, o2, bits(d2, 64), -1.0, 0.0)]
        cases.append((name, planted_frame(feats), planted_mp([(100.0, 75.0, 60.0, 1, Z, 1, 1, V)]),
                      lambda nm, row, st, want=want: nm == want and row[0] == (0 if want else -1)))
    # u_right exactly at the radius passes, one ulp further does not (the better descriptor then loses)
    for name, urf, want in (("u_right-at-radius", F32(60.0 - 12.0), 0), ("u_right-past-radius", np.nextafter(F32(48.0), F32(-1e9)), 1)):
        feats = [(100.0, 75.0, 0, bits(1), urf, 0.0), (101.0, 75.0, 0, bits(30), F32(61.0), 0.0)]
        cases.append((name, planted_frame(feats), planted_mp([(100.0, 75.0, 60.0, 0, Z, 1, 1, V)]),
                      lambda nm, row, st, want=want: nm == 1 and row[want] == 0))
    # a bucket of 70 with ties; a window over the grid edge
    feats = [(50.0 + 0.01 * i, 50.0, 0, bits(40 if i not in (3, 66) else 1, i), -1.0, 0.0) for i in range(70)]
    cases.append(("bucket>64", planted_frame(feats), planted_mp([(50.0, 50.0, 10.0, 0, Z, 1, 1, V)], th=1.0),
                  lambda nm, row, st: nm == 0 and st["ratio_rejects"] == 1))          # best == second (1, 1) on one level
    feats = [(1.0 + 4.0 * i, 2.0 + 3.0 * (i % 5), 2, bits(2 + 7 * i), -1.0, 0.0) for i in range(12)]
    cases.append(("over-the-edge", planted_frame(feats), planted_mp([(2.0, 3.0, 1.0, 2, Z, 1, 1, V)], th=5.0),
                  lambda nm, row, st: nm == 1 and row[0] == 0))
    # two observed points want one feature; a feature that is occupied from the start; the second best blocked alone
    feats = [(100.0, 75.0, 0, bits(2), -1.0, 0.0), (102.0, 75.0, 0, bits(30), -1.0, 0.0)]
    cases.append(("blocked-rescan", planted_frame(feats),
                  planted_mp([(100.0, 75.0, 60.0, 0, Z, 2, 1, V), (101.0, 75.0, 60.0, 0, Z, 2, 1, V)]),
                  lambda nm, row, st: nm == 2 and row[0] == 0 and row[1] == 1 and st["rescans"] == 1))
    fo = np.full(CAP, -1, np.int32); fo[0] = 3
    cases.append(("seeded-occupied", planted_frame(feats), planted_mp([(100.0, 75.0, 60.0, 0, Z, 2, 1, V)], frame_observations=fo),
                  lambda nm, row, st: nm == 1 and row[0] == -1 and row[1] == 0 and st["rescans"] == 1))
    fo = np.full(CAP, -1, np.int32); fo[1] = 1                        # without its second best the ratio test has nothing to fail on
    feats = [(100.0, 75.0, 0, bits(9), -1.0, 0.0), (102.0, 75.0, 0, bits(10, 64), -1.0, 0.0)]
    cases.append(("second-blocked", planted_frame(feats), planted_mp([(100.0, 75.0, 60.0, 0, Z, 2, 1, V)], frame_observations=fo),
                  lambda nm, row, st: nm == 1 and row[0] == 0 and st["rescans"] == 1))
    # a 0-observation point does not block: the later point takes the feature over
    feats = [(100.0, 75.0, 0, bits(2), -1.0, 0.0)]
    cases.append(("override", planted_frame(feats),
                  planted_mp([(100.0, 75.0, 60.0, 0, Z, 0, 1, V), (101.0, 75.0, 60.0, 0, Z, 1, 1, V)]),
                  lambda nm, row, st: nm == 2 and row[0] == 1 and st["rescans"] == 0))
    # degenerate problems
    pts = [(100.0, 75.0, 60.0, 0, Z, 1, 1, V)] * 3
    cases.append(("count-0", planted_frame([]), planted_mp(pts), lambda nm, row, st: nm == 0))
    cases.append(("view-n-0", planted_frame(feats), planted_mp([]), lambda nm, row, st: nm == 0 and (row == -1).all()))
    cases.append(("none-in-view", planted_frame(feats), planted_mp([(100.0, 75.0, 60.0, 0, Z, 1, 0, V)] * 3),
                  lambda nm, row, st: nm == 0 and (row == -1).all()))
    return cases


def test_mappoint_policy_planted_edges(exfp):
    ex, fp, scale = exfp
    cases = planted_mp_cases()
    rng = np.random.default_rng(10)
    full = tm.make_frame(rng, CAP)
    cases.append(("count==cap", full, tm.make_mp_problem(rng, full, 300, cap=CAP), lambda nm, row, st: nm > 50 and st["rescans"] > 0))
    frames = [c[1] for c in cases]
    probs = [dict(c[2], frame=i) for i, c in enumerate(cases)]
    probs.append(dict(probs[-1], th=F32(5.0)))                      # the same frame in two problems
    batch = DeviceBatch(ex, frames)
    nm, rows = check_mp(ex, batch, probs, 0.8, scale, "planted")
    for i, (name, fr, p, expect) in enumerate(cases):
        po = p if p["frame_observations"] is not None else dict(p, frame_observations=np.full(CAP, -1, np.int32))
        st = tm.model_mp(fr, po, 0.8, scale)[2]
        assert expect(int(nm[i]), rows[i, :len(fr["keys"])], st), (name, int(nm[i]), st, rows[i, :len(fr["keys"])][:30])
    assert nm[-1] > 50


# ----------------------------------------------------------------------------------------------- determinism, asynchrony
def test_determinism_and_asynchrony(exfp, random_frames):
    """two calls give byte-equal outputs; the host arrays may be overwritten as soon as the call has returned (they were
    packed into the staging block), also by a second call issued behind the first without a synchronisation in between"""
    ex, fp, scale = exfp
    batch = DeviceBatch(ex, random_frames)
    rng = np.random.default_rng(505)
    fprobs = [dict(tm.make_ff_problem(rng, random_frames[f], 300, motion="forward", th=15.0, scale=scale), frame=f) for f in (0, 1, 0)]
    mprobs = [dict(tm.make_mp_problem(rng, random_frames[f], 300, cap=CAP), frame=f) for f in (0, 1, 0)]
    a = run_ff(ex, batch, fprobs, True); b = run_ff(ex, batch, fprobs, True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0].sum() > 50
    c = run_mp(ex, batch, mprobs, 0.8); d = run_mp(ex, batch, mprobs, 0.8)
    assert c[0].tobytes() == d[0].tobytes() and c[1].tobytes() == d[1].tobytes() and c[0].sum() > 50
    # overwrite every host array right after the calls return, synchronise afterwards
    m = ORBmatcher(0.8, True, extractor=ex)
    fcopy = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()} for p in fprobs]
    mcopy = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()} for p in mprobs]
    frows, fnm = batch.outputs(3); mrows, mnm = batch.outputs(3)
    m.SearchByProjectionBatchDevice(fcopy, batch.args(), K=tm.CAMERA, mb=tm.MB, mbf=tm.MBF, d_matched_last=frows, d_nmatches=fnm)
    m.SearchByProjectionMapPointsBatchDevice(mcopy, batch.args(), d_assigned=mrows, d_nmatches=mnm)
    for p in fcopy + mcopy:
        for v in p.values():
            if isinstance(v, np.ndarray):
                v.view(np.uint8).reshape(-1)[:] = 0xa5
    ex.synchronize()
    assert fnm.cpu().numpy().tobytes() == a[0].tobytes() and frows.cpu().numpy().tobytes() == a[1].tobytes()
    assert mnm.cpu().numpy().tobytes() == c[0].tobytes() and mrows.cpu().numpy().tobytes() == c[1].tobytes()


# ----------------------------------------------------------------------------------------------- end to end
def test_end_to_end_chain(exfp):
    """extract_batch_device -> undistort_keypoints_device -> grid_build_device -> the batched frame call, on 4 frames of a
    synthetic stream; compared with the single call fed the downloaded buffers"""
    import torch
    ex0, fp, scale = exfp
    L = _capi.lib()
    W, H, B = 320, 240, 4
    ex = ORBextractor(500, 1.2, 8, 20, 7, fp_mode=fp, max_batch=B)
    img = synth.stream(W, H, B, stream_id=7)
    dev = torch.device("cuda", 0)
    cap = ex.max_keypoints(W, H)
    d_img = torch.from_numpy(img).to(dev)
    kps = torch.zeros((B, cap * 28), dtype=torch.uint8, device=dev); kun = torch.zeros((B, cap * 28), dtype=torch.uint8, device=dev)
    desc = torch.zeros((B, cap * 32), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev); st = torch.zeros(B, dtype=torch.int32, device=dev)
    cb = torch.zeros((B, 64 * 48 + 1), dtype=torch.int32, device=dev); it = torch.zeros((B, cap), dtype=torch.int16, device=dev)
    rows = torch.full((B, cap), SENTINEL, dtype=torch.int32, device=dev); nm = torch.full((B,), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    K4 = np.array([260.0, 260.0, 160.0, 120.0], np.float32); dist = np.array([-0.05, 0.01, 0.0005, -0.0003, 0.0], np.float32)
    b4 = np.zeros(4, np.float32)
    _capi.check(L.orbx_image_bounds(ex.handle, W, H, _capi.ptr(K4), _capi.ptr(dist), 5, _capi.ptr(b4)))
    # the last frame of every problem: MapPoints a metre and more in front of an identity camera, seen by frame 0
    k0, d0 = ex.extract_batch(img[:1])[0]
    k0u = k0.copy()
    rng = np.random.default_rng(8)
    z = rng.uniform(2.0, 6.0, len(k0)).astype(np.float32)
    xw = np.stack([(k0["x"] - K4[2]) / K4[0] * z, (k0["y"] - K4[3]) / K4[1] * z, z], 1).astype(np.float32)
    Tlw = np.eye(4, dtype=np.float32); Tlw[2, 3] = 0.3
    probs = [dict(frame=f, th=F32(15.0 if f < 3 else 30.0), mono=int(f == 1), Tcw=np.eye(4, dtype=np.float32), Tlw=Tlw, keys_un=k0u,
                  has_map_point=(rng.uniform(size=len(k0)) < 0.9).astype(np.uint8), world_pos=xw, mp_desc=d0,
                  observations=rng.choice([0, 1, 2], len(k0)).astype(np.int32)) for f in range(B)]
    ex.extract_batch_device(d_img, B, W, H, W, W * H, kps, desc, cnt, st, cap)
    _capi.check(L.orbx_undistort_keypoints_device(ex.handle, B, _capi.ptr(kps), _capi.ptr(cnt), cap, _capi.ptr(K4), _capi.ptr(dist), 5,
                                                  _capi.ptr(kun)))
    _capi.check(L.orbx_grid_build_device(ex.handle, B, _capi.ptr(kun), _capi.ptr(cnt), cap, _capi.ptr(b4), _capi.ptr(cb), _capi.ptr(it)))
    m = ORBmatcher(0.8, True, extractor=ex)
    m.SearchByProjectionBatchDevice(probs, dict(nframes=B, keys_un=kun, desc=desc, u_right=None, counts=cnt, cap=cap, cell_begin=cb,
                                                items=it, bounds=tuple(float(v) for v in b4)),
                                    K=K4, mb=0.1, mbf=40.0, d_matched_last=rows, d_nmatches=nm)
    ex.synchronize()
    cnt_h, nm_h, rows_h = cnt.cpu().numpy(), nm.cpu().numpy(), rows.cpu().numpy()
    kun_h = kun.cpu().numpy().view(_capi.KP_DTYPE).reshape(B, cap); desc_h = desc.cpu().numpy().reshape(B, cap, 32)
    total = 0
    for f in range(B):
        n = int(cnt_h[f])
        cur = types.SimpleNamespace(mvKeysUn=np.ascontiguousarray(kun_h[f, :n]), mDescriptors=np.ascontiguousarray(desc_h[f, :n]),
                                    mvuRight=np.full(n, -1.0, np.float32), N=n, bounds=tuple(float(v) for v in b4))
        last = types.SimpleNamespace(mvKeysUn=k0u, N=len(k0u))
        p = probs[f]
        sn, sm = m.SearchByProjection(cur, last, float(p["th"]), p["mono"], Tcw=p["Tcw"], Tlw=p["Tlw"], K=K4, mb=0.1, mbf=40.0,
                                      has_map_point=p["has_map_point"], world_pos=p["world_pos"], mp_desc=p["mp_desc"],
                                      observations=p["observations"])
        print(f"chain frame {f}: {n} keypoints, nmatches {nm_h[f]} single {sn}")
        assert nm_h[f] == sn and np.array_equal(rows_h[f, :n], sm) and (rows_h[f, n:] == SENTINEL).all()
        total += int(sn)
    assert total > 100
    ex.close()
