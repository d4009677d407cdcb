"""MapPoint::ComputeDistinctiveDescriptors / MapPoint::UpdateNormalAndDepth for a ragged batch of points
(include/orbx.h: orbx_distinctive_descriptors_batch, orbx_distinctive_descriptors_batch_device,
orbx_update_normal_and_depth_batch).  ctypes marshalling only; `extractor` is the ORBextractor whose handle (stream, scale
tables) the calls run on.  Point p owns the rows obs_begin[p] .. obs_begin[p + 1], in the iteration order of the caller's
std::map<KeyFrame*, size_t>: that order decides between equal medians."""
from __future__ import annotations

import numpy as np

from . import _capi
from ._capi import check, ptr


def _outputs(npoints, best_desc):
    idx, med = np.full(npoints, -1, np.int32), np.full(npoints, -1, np.int32)
    if best_desc is None:
        best_desc = np.zeros((npoints, 32), np.uint8)
    assert best_desc.dtype == np.uint8 and best_desc.flags.c_contiguous and best_desc.size == npoints * 32
    return idx, med, best_desc


def distinctive_descriptors_batch(extractor, obs_begin, desc, best_desc=None):
    """desc [obs_begin[-1], 32] uint8 on the host, bad keyframes already left out.  Returns (best_idx, best_median, best_desc);
    a point without rows gets -1, -1 and keeps its row of best_desc (the caller's array when one is passed: it is written in
    place)."""
    ob = np.ascontiguousarray(obs_begin, np.int32)
    d = np.ascontiguousarray(desc, np.uint8)
    npoints = len(ob) - 1
    idx, med, out = _outputs(max(npoints, 0), best_desc)
    check(_capi.lib().orbx_distinctive_descriptors_batch(extractor.handle, npoints, ptr(ob), ptr(d) if d.size else None, ptr(idx),
                                                         ptr(med), ptr(out)))
    return idx, med, out


def distinctive_descriptors_batch_device(extractor, d_pool, pool_rows, obs_begin, obs_row, best_desc=None):
    """the same with the rows named: row t is d_pool[obs_row[t]], d_pool a device buffer (torch tensor or address) of
    pool_rows x 32 bytes.  Results on the host."""
    ob = np.ascontiguousarray(obs_begin, np.int32)
    rows = np.ascontiguousarray(obs_row, np.int64)
    npoints = len(ob) - 1
    idx, med, out = _outputs(max(npoints, 0), best_desc)
    check(_capi.lib().orbx_distinctive_descriptors_batch_device(extractor.handle, ptr(d_pool), int(pool_rows), npoints, ptr(ob),
                                                                ptr(rows) if rows.size else None, ptr(idx), ptr(med), ptr(out)))
    return idx, med, out


def update_normal_and_depth_batch(extractor, obs_begin, pos, centers, ref_center, ref_level, normal=None, min_distance=None,
                                  max_distance=None):
    """pos / ref_center [P, 3], centers [obs_begin[-1], 3] = GetCameraCenter() of every observing keyframe in the map's order, bad
    ones included, ref_level [P].  Returns (normal [P, 3], min_distance [P], max_distance [P]); a point without rows keeps its
    entries (the caller's arrays when passed: they are written in place; zeros otherwise)."""
    ob = np.ascontiguousarray(obs_begin, np.int32)
    npoints = max(len(ob) - 1, 0)
    a = [np.ascontiguousarray(x, np.float32) for x in (pos, centers, ref_center)]
    lvl = np.ascontiguousarray(ref_level, np.int32)
    normal = np.zeros((npoints, 3), np.float32) if normal is None else normal
    min_distance = np.zeros(npoints, np.float32) if min_distance is None else min_distance
    max_distance = np.zeros(npoints, np.float32) if max_distance is None else max_distance
    for x in (normal, min_distance, max_distance):
        assert x.dtype == np.float32 and x.flags.c_contiguous
    check(_capi.lib().orbx_update_normal_and_depth_batch(extractor.handle, len(ob) - 1, ptr(ob), ptr(a[0]),
                                                         ptr(a[1]) if a[1].size else None, ptr(a[2]), ptr(lvl), ptr(normal),
                                                         ptr(min_distance), ptr(max_distance)))
    return normal, min_distance, max_distance
