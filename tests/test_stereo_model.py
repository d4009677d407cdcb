"""tests/stereo_model.py (Frame::ComputeStereoMatches, src/Frame.cc:880-1176, written from the reference text) against the oracle's
orc_stereo_matches on the planted scenes of tests/stereo_scenes.py and on ordinary extractions.  No GPU.

Non-vacuity is asserted, not reported: every planted keypoint leaves the function at the line the scene planted it for, every
reason code occurs, the median-cut scenes keep and drop.

DELTA_RANGE (:1128) cannot occur.  dist2 is the FIRST minimum of the 11 SADs and bestincR is not at an end (:1105), so with
a = dist1 - dist2 > 0 (strict: an equal earlier value would have been the first minimum) and b = dist3 - dist2 >= 0 the quotient is
(a - b) / (2 (a + b)), inside [-0.5, 0.5]; the denominator is never 0, so no NaN either.  SADs are integers below 2^16, so float
evaluates all of it exactly up to the one division.  test_every_reason_code_occurs asserts that no scene reaches the code
instead of inventing a case."""
import numpy as np
import pytest

import oracle
import stereo_model as sm
import stereo_scenes as S
from orb_slam2_detailed_comments_amd import synth

_seen = {}


def run(s, pyr):
    res = sm.stereo_model(s.kL, s.dL, s.kR, s.dR, s.scale, s.inv, pyr[0], pyr[1], s.mb, s.mbf)
    on, ou, od = oracle.stereo_matches(s.kL, s.dL, s.kR, s.dR, s.scale, s.inv, pyr[0], pyr[1], s.mb, s.mbf)
    n, u, d, sad, reason = res
    assert n == on
    assert np.array_equal(u.view(np.uint32), ou.view(np.uint32))
    assert np.array_equal(d.view(np.uint32), od.view(np.uint32))
    return res


check_planted = S.check_planted


@pytest.mark.parametrize("name", S.SMALL_NAMES)
def test_planted_scene(name):
    s = S.small_scenes()[name]
    assert (s.W[0], s.H[0]) == ((s.w + 38, s.h + 38) if s.mode == "fork" else (s.w, s.h))
    pyr = S.cpu_pyramids(name)
    assert [a.shape for a in pyr[0]] == list(zip(s.H, s.W))
    res = run(s, pyr)
    check_planted(s, res)
    assert (s.reason >= 0).any()
    _seen[name] = set(res[4].tolist())


def test_tall_scene():
    """matches, bounds and row cuts down 2758 rows, the last ones included"""
    s = S.tall_scene()
    pyr = S.cpu_pyramids(s.name)
    assert pyr[0][0].shape == (S.TALL_H + 38, S.TALL_W + 38)
    res = run(s, pyr)
    check_planted(s, res)
    assert (s.kL["y"][np.isin(res[4], (sm.MATCHED,))] > S.TALL_H).any()


def test_every_reason_code_occurs():
    seen = set()
    for name in S.SMALL_NAMES:
        if name not in _seen:      # run alone: compute what test_planted_scene would have left
            s = S.small_scenes()[name]
            _seen[name] = set(sm.stereo_model(s.kL, s.dL, s.kR, s.dR, s.scale, s.inv, *S.cpu_pyramids(name), s.mb, s.mbf)[4].tolist())
        seen |= _seen[name]
    codes = set(sm.NAMES)
    assert seen == codes - {sm.DELTA_RANGE}, sorted(sm.NAMES[c] for c in codes ^ seen)   # module docstring: :1128 is unreachable
    planted = set()
    for s in S.small_scenes().values():
        planted |= set(s.reason[s.reason >= 0].tolist())
    assert planted == codes - {sm.DELTA_RANGE}


def test_median_sets_are_what_they_say():
    """the planted SADs come back as the SADs"""
    for which, (sads, copies, cut) in S.MEDIAN_SETS.items():
        s = S.small_scenes()["median_%s_upstream_96x64" % which]
        sad = sm.stereo_model(s.kL, s.dL, s.kR, s.dR, s.scale, s.inv, *S.cpu_pyramids(s.name), s.mb, s.mbf)[3]
        assert sad.tolist() == sads * copies
    assert len(S.small_scenes()["median_many_fork_160x120"].kL) > 256


@pytest.mark.parametrize("sid", [7, 8])
def test_model_on_extracted_keypoints(sid):
    L, R = synth.stereo_pair(320, 240, stream_id=sid)
    eL, eR = oracle.OracleExtractor(400), oracle.OracleExtractor(400)
    nL, kL, dL = eL.extract(L)
    nR, kR, dR = eR.extract(R)
    t = eL.tables()
    pyrL = [eL.level_image(l) for l in range(8)]
    pyrR = [eR.level_image(l) for l in range(8)]
    n, u, d, sad, reason = sm.stereo_model(kL, dL, kR, dR, t["scale"], t["inv_scale"], pyrL, pyrR, 0.1, 30.0)
    on, ou, od = oracle.stereo_matches(kL, dL, kR, dR, t["scale"], t["inv_scale"], pyrL, pyrR, 0.1, 30.0)
    assert n == on and n > 20
    assert np.array_equal(u.view(np.uint32), ou.view(np.uint32)) and np.array_equal(d.view(np.uint32), od.view(np.uint32))
    assert not (reason == sm.DELTA_RANGE).any() and (reason == sm.CUT).any()
