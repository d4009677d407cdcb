"""compat/MapPoint_batch.inl (MapPoint::RefreshBatch) through the stand-ins of tests/compat_mappoint/: a scene of about 300
points over 12 keyframes -- a bad point, an unobserved point, a bad keyframe, a point seen by that keyframe alone, a duplicated
list entry and a NULL -- played once through the loop of single ComputeDistinctiveDescriptors() + UpdateNormalAndDepth() calls
and once through RefreshBatch on the device; every point's descriptor, normal and distance bounds are compared byte for byte,
with each other and with tests/mappoint_model.py.  The syntax-only compile needs neither the library nor a GPU."""
import shutil
import subprocess

import numpy as np
import pytest

import mappoint_harness as mh


def test_compat_mappoint_syntax():
    assert shutil.which("g++")
    p = subprocess.run(mh.build_cmd(None, syntax_only=True), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]


@pytest.mark.gpu
@pytest.mark.parametrize("parts", [(1, 1), (1, 0), (0, 1)])
def test_refresh_batch_equals_the_loop_of_single_calls(built_lib, tmp_path, parts):
    M = mh.build(str(tmp_path / "compat_mappoint.so"))
    pts, kfs, order = mh.play_scene(M)
    M.call("mpt_single_loop", order, len(order), *parts)
    loop_d, loop_o = M.states(len(pts))
    M.restore(pts)                                                   # the same map (and map order), its points as they were
    pts2, kfs2 = pts, kfs
    before_d, before_o = M.states(len(pts))
    assert np.array_equal(before_d, np.stack([P["desc"] for P in pts]))
    M.call("mpt_refresh_batch", order, len(order), *parts)
    d, o = M.states(len(pts))
    assert np.array_equal(d, loop_d)
    assert np.array_equal(o.view(np.uint32), loop_o.view(np.uint32))
    md, mo = mh.model_scene(M, pts2, kfs2)
    assert np.array_equal(d, md if parts[0] else before_d)
    assert np.array_equal(o.view(np.uint32), (mo if parts[1] else before_o).view(np.uint32))
    for p in (5, 7):                                                 # unobserved, bad: left as they were
        assert np.array_equal(d[p], before_d[p]) and np.array_equal(o[p].view(np.uint32), before_o[p].view(np.uint32))
    assert np.array_equal(d[9], before_d[9])                         # seen by the bad keyframe alone: no descriptor ...
    if parts[1]:
        assert not np.array_equal(o[9], before_o[9])                 # ... but its normal is refreshed
    assert (d != before_d).any() or not parts[0]
