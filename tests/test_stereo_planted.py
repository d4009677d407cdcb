"""The stereo kernels (k_stereo, k_stereo_batch, k_stereo_rows, k_stereo_cut and the host cut of orbx_stereo_match) on the planted
scenes of tests/stereo_scenes.py, bit for bit against tests/stereo_model.py run on the pyramid levels read back from the handles.

Keypoints and descriptors are caller data, so the scenes put them where extracted keypoints never are: on every edge of the patch
and search-window checks, on the edges of every gate, on row 0 and the last row, past row 4096.  Each scene goes through
Frame.ComputeStereoMatches (frames 0 / 0 and 2 / 1 of three-image batches), orbx_stereo_match_batch_device on two handles and on
one handle that extracted both eyes (B = 3: one pair without right keypoints, one without left keypoints, the scene itself as the
last pair with a count that claims more than `cap`)."""
import numpy as np
import pytest

import stereo_model as sm
import stereo_scenes as S
from orb_slam2_detailed_comments_amd import ORBextractor, OrbxError, Frame, _capi

pytestmark = pytest.mark.gpu
KP = _capi.KP_DTYPE
SENTINEL = 7.0


def extractor(s, max_batch, fp=_capi.FP_GCC_FMA):
    mode = _capi.PYRAMID_UPSTREAM if s.mode == "upstream" else _capi.PYRAMID_FORK_PADDED
    return ORBextractor(100, s.factor, s.nlevels, 20, 7, max_batch=max_batch, fp_mode=fp, pyramid_mode=mode)


def fillers(s, n=4):
    rng = np.random.default_rng(99)
    return [rng.integers(0, 256, (s.h, s.w)).astype(np.uint8) for _ in range(n)]


def levels(ex, s, frame):
    return [ex.pyramid_level(l, frame) for l in range(s.nlevels)]


def model(s, exL, fl, exR, fr):
    """the model on what the handles hold; the planted keypoints must be on target there as well"""
    res = sm.stereo_model(s.kL, s.dL, s.kR, s.dR, exL.GetScaleFactors(), exL.GetInverseScaleFactors(), levels(exL, s, fl),
                          levels(exR, s, fr), s.mb, s.mbf)
    S.check_planted(s, res)
    return res


def assert_bits(got, ref, what):
    n, u, d = got
    assert n == ref[0], what
    assert np.array_equal(u.view(np.uint32), ref[1].view(np.uint32)), what
    assert np.array_equal(d.view(np.uint32), ref[2].view(np.uint32)), what


def single(s, exL, exR, fl, fr):
    FL, FR = Frame(s.kL, s.dL, s.w, s.h), Frame(s.kR, s.dR, s.w, s.h)
    n = FL.ComputeStereoMatches(FR, exL, exR, s.mb, s.mbf, fl, fr)
    return n, FL.mvuRight, FL.mvDepth


def extract_device(ex, imgs):
    """one orbx_extract_batch_device call; only the pyramids it leaves are used"""
    import torch
    dev = torch.device("cuda", 0)
    b, (h, w) = len(imgs), imgs[0].shape
    cap = ex.max_keypoints(w, h)
    t = torch.from_numpy(np.stack(imgs)).to(dev)
    kps = torch.zeros((b, cap * 28), dtype=torch.uint8, device=dev); desc = torch.zeros((b, cap * 32), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(b, dtype=torch.int32, device=dev); st = torch.zeros(b, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()   # fills ran on torch's stream; the handle's stream is not ordered with it
    ex.extract_batch_device(t, b, w, h, w, w * h, kps, desc, cnt, st, cap)
    ex.synchronize()
    assert not st.cpu().numpy().any()


def batched(s, hl, hr, pairs, cap):
    """pairs: (kL, dL, countL, kR, dR, countR) per pair, the counts as the count buffers state them.  Returns per pair
    (nmatches, uRight[:n], depth[:n]) with n = min(countL, cap), after checking that nothing past n was written."""
    import torch
    dev = torch.device("cuda", 0)
    B = len(pairs)

    def up(ks, ds):
        kb = np.zeros((B, cap), KP); db = np.zeros((B, cap, 32), np.uint8)
        for p, (k, d) in enumerate(zip(ks, ds)):
            kb[p, :len(k)] = k
            db[p, :len(k)] = d
        return (torch.from_numpy(kb.view(np.uint8).reshape(B, cap * 28)).to(dev), torch.from_numpy(db.reshape(B, cap * 32)).to(dev))

    tkl, tdl = up([p[0] for p in pairs], [p[1] for p in pairs])
    tkr, tdr = up([p[3] for p in pairs], [p[4] for p in pairs])
    cl = torch.tensor([p[2] for p in pairs], dtype=torch.int32, device=dev)
    cr = torch.tensor([p[5] for p in pairs], dtype=torch.int32, device=dev)
    ur = torch.full((B, cap), SENTINEL, dtype=torch.float32, device=dev); dep = torch.full((B, cap), SENTINEL, dtype=torch.float32, device=dev)
    nm = torch.full((B,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _capi.check(_capi.lib().orbx_stereo_match_batch_device(hl.handle, hr.handle, B, _capi.ptr(tkl), _capi.ptr(tdl), _capi.ptr(cl),
                                                           _capi.ptr(tkr), _capi.ptr(tdr), _capi.ptr(cr), cap, s.mb, s.mbf,
                                                           _capi.ptr(ur), _capi.ptr(dep), _capi.ptr(nm)))
    hl.synchronize()
    ur, dep, nm = ur.cpu().numpy(), dep.cpu().numpy(), nm.cpu().numpy()
    out = []
    for p in range(B):
        n = min(pairs[p][2], cap)
        assert (ur[p, n:] == SENTINEL).all() and (dep[p, n:] == SENTINEL).all()
        out.append((int(nm[p]), ur[p, :n].copy(), dep[p, :n].copy()))
    return out


def three_pairs(s):
    """B = 3: left keypoints without a right one, right keypoints without a left one, and the scene with a count past cap"""
    nL, nR = len(s.kL), len(s.kR)
    cap = max(nL, nR, 1)
    over = (nL + 3 if nL == cap else nL, nR + 3 if nR == cap else nR)
    assert over[0] > cap or over[1] > cap
    return cap, [(s.kL, s.dL, nL, s.kR[:0], s.dR[:0], 0), (s.kL[:0], s.dL[:0], 0, s.kR, s.dR, nR),
                 (s.kL, s.dL, over[0], s.kR, s.dR, over[1])]


def check_batched(s, out, ref, what):
    nL = len(s.kL)
    none = (0, np.full(nL, -1.0, np.float32), np.full(nL, -1.0, np.float32))
    assert_bits(out[0], none, what + ": no right keypoints")
    assert_bits(out[1], (0, np.zeros(0, np.float32), np.zeros(0, np.float32)), what + ": no left keypoints")
    assert_bits(out[2], ref, what)


@pytest.mark.parametrize("name", S.SMALL_NAMES)
def test_planted_scene(name):
    s = S.small_scenes()[name]
    O = fillers(s)
    exL, exR = extractor(s, 3), extractor(s, 3)
    # single form, frames 2 / 1 of two three-image batches
    exL.extract_batch(np.stack([O[0], O[1], s.imgL]))
    exR.extract_batch(np.stack([O[2], s.imgR, O[3]]))
    assert exL.pyramid_level(0, 2).shape == (s.H[0], s.W[0])
    ref = model(s, exL, 2, exR, 1)
    one = single(s, exL, exR, 2, 1)
    assert_bits(one, ref, "single form, frames 2 / 1")
    # frames 0 / 0
    exL.extract_batch(np.stack([s.imgL, O[0], O[1]]))
    exR.extract_batch(np.stack([s.imgR, O[2], O[3]]))
    assert_bits(single(s, exL, exR, 0, 0), ref, "single form, frames 0 / 0")
    # batched, two handles: the scene is pair 2
    cap, pairs = three_pairs(s)
    extract_device(exL, [O[0], O[1], s.imgL])
    extract_device(exR, [O[2], O[3], s.imgR])
    two = batched(s, exL, exR, pairs, cap)
    check_batched(s, two, ref, "batched, two handles")
    assert_bits(two[2], one, "host cut against k_stereo_cut")
    # batched, one handle that extracted both eyes
    ex = extractor(s, 6)
    extract_device(ex, [O[0], O[1], s.imgL, O[2], O[3], s.imgR])
    check_batched(s, batched(s, ex, ex, pairs, cap), ref, "batched, one handle")


@pytest.mark.parametrize("name", ["disparity_fork_160x120", "bounds_upstream_96x64_cols_3"])
def test_fp_mode_does_not_enter(name):
    s = S.small_scenes()[name]
    out = []
    for fp in (_capi.FP_GCC_FMA, _capi.FP_STRICT):
        exL, exR = extractor(s, 1, fp), extractor(s, 1, fp)
        exL(s.imgL); exR(s.imgR)
        out.append(single(s, exL, exR, 0, 0))
        assert_bits(out[-1], model(s, exL, 0, exR, 0), "fp_mode %d" % fp)
    assert_bits(out[0], out[1], "the two fp_modes")


def test_tall_pair():
    """2758 rows: the row table of k_stereo_rows near the tallest level 0 the library takes.  One extraction per eye."""
    s = S.tall_scene()
    exL, exR = extractor(s, 1), extractor(s, 1)
    extract_device(exL, [s.imgL])
    extract_device(exR, [s.imgR])
    assert exL.pyramid_level(0).shape == (S.TALL_H + 38, S.TALL_W + 38)
    ref = model(s, exL, 0, exR, 0)
    one = single(s, exL, exR, 0, 0)
    assert_bits(one, ref, "single form")
    nL, nR = len(s.kL), len(s.kR)
    assert nL > nR
    two = batched(s, exL, exR, [(s.kL, s.dL, nL + 3, s.kR, s.dR, nR)], nL)
    assert_bits(two[0], ref, "batched form")


def test_no_level_0_reaches_the_brute_force_rows():
    """orbx_stereo_body walks every right keypoint itself when nrows0 > 4096 (k_stereo_rows holds 4096 rows in LDS).  No image gets
    there: a level has at most 4095 FAST cells and an aspect ratio of at least 0.5, which ends below 2.8 k rows.  If either limit is
    lifted this fails, and that path then needs the tall scene at 2112 x 4060 (4098 rows) and at 2112 x 4058 (4096)."""
    ex = ORBextractor(100, 1.2, 2, 20, 7)
    for w, h in ((2112, 4060), (2112, 4058), (1360, 4060), (2112, 3000)):
        with pytest.raises(OrbxError) as e:
            ex.max_keypoints(w, h)
        assert e.value.status in (_capi.UNSUPPORTED, _capi.BAD_ASPECT)
