"""LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:336-680): the per-match geometry of :450-651 as one batched call
(orbx_create_new_map_points_batch, k_new_points) and the neighbour loop of :378-679 for many streams at once.

A keyframe is a dict: Rcw [3, 3], tcw [3], Ow [3] (GetRotation, GetTranslation, GetCameraCenter as the keyframe holds them), fx,
fy, cx, cy, invfx, invfy, mb, mbf, scale_factors and level_sigma2 (mvScaleFactors, mvLevelSigma2), keys_un (KP_DTYPE, mvKeysUn),
keys [n, 2] (mvKeys pt, the distorted positions KeyFrame::UnprojectStereo reads), u_right and depth [n] (mvuRight, mvDepth); the
current keyframe also scale_factor (mfScaleFactor).  The rounds driver reads has_map_point [n] too, and the default selection
the fields ORBmatcher's keyframe views need (desc, feat_vec)."""
from __future__ import annotations
import numpy as np
from . import _capi
from ._capi import check

ACCEPTED = (_capi.NEWPOINT_TRIANGULATED, _capi.NEWPOINT_STEREO1, _capi.NEWPOINT_STEREO2)


def _keyframe(kf, out, keep):
    a = lambda x, t: np.ascontiguousarray(x, t)
    for name, size in (("Rcw", 9), ("tcw", 3), ("Ow", 3)):
        v = a(kf[name], np.float32).reshape(-1)
        if v.size != size:
            raise ValueError(f"{name} must have {size} entries")
        getattr(out, name)[:] = v.tolist()
    for name in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf"):
        setattr(out, name, float(np.float32(kf[name])))
    sf, ls = a(kf["scale_factors"], np.float32), a(kf["level_sigma2"], np.float32)
    if len(sf) != len(ls):
        raise ValueError("scale_factors and level_sigma2 must have the same length")
    keys_un, keys = a(kf["keys_un"], _capi.KP_DTYPE), a(kf["keys"], np.float32).reshape(-1, 2)
    ur, depth = a(kf["u_right"], np.float32), a(kf["depth"], np.float32)
    if not (len(keys_un) == len(keys) == len(ur) == len(depth)):
        raise ValueError("keys_un, keys, u_right and depth must have one entry per feature")
    keep += [sf, ls, keys_un, keys, ur, depth]
    out.nlevels, out.scale_factors, out.level_sigma2 = len(sf), sf.ctypes.data, ls.ctypes.data
    out.n, out.keys_un, out.keys, out.u_right, out.depth = len(keys_un), keys_un.ctypes.data, keys.ctypes.data, ur.ctypes.data, depth.ctypes.data


def _newpoints_marshal(problems):
    """the orbx_newpoints_problem array of a call, the arrays it points into, and the match counts"""
    K = len(problems)
    arr = (_capi.NewPointsProblem * max(K, 1))()
    keep, counts = [], []
    for k, p in enumerate(problems):
        m = np.ascontiguousarray(p["matches"], np.int32).reshape(-1, 2)
        keep.append(m)
        _keyframe(p["kf1"], arr[k].kf1, keep)
        _keyframe(p["kf2"], arr[k].kf2, keep)
        arr[k].scale_factor = float(np.float32(p["kf1"]["scale_factor"]))
        arr[k].nmatches, arr[k].matches = len(m), m.ctypes.data
        counts.append(len(m))
    return arr, keep, counts


def create_new_map_points_batch(ex, problems):
    """problems: [{"kf1": keyframe, "kf2": keyframe, "matches": int32 [n, 2] (vMatchedIndices in order)}], each ONE (current
    keyframe, neighbour) pair.  One device round trip for all of them (on a host-only extractor, or with ORBX_NEWPOINTS=host in the
    environment, the library's host path).  Returns per problem (status uint8 [n], points float32 [n, 3]): status is one of
    _capi.NEWPOINT_*, 1..3 accept, and the point of a rejected match is zero."""
    arr, keep, counts = _newpoints_marshal(problems)
    total = sum(counts)
    status = np.zeros(max(total, 1), np.uint8)
    points = np.zeros((max(total, 1), 3), np.float32)
    check(_capi.lib().orbx_create_new_map_points_batch(ex.handle, len(problems), arr, _capi.ptr(status), _capi.ptr(points)))
    out, off = [], 0
    for n in counts:
        out.append((status[off:off + n].copy(), points[off:off + n].copy()))
        off += n
    return out


def matched_pairs(matches12):
    """vMatchedIndices of SearchForTriangulation from its matches12 [KF1.N]: (idx1, idx2) in ascending idx1"""
    m = np.asarray(matches12, np.int32)
    i = np.nonzero(m >= 0)[0].astype(np.int32)
    return np.stack([i, m[i]], axis=1) if len(i) else np.zeros((0, 2), np.int32)


def _default_select(ex, stream):
    """SearchForTriangulation through ORBmatcher.TriangulationBatch: the distances of all neighbours that are not skipped now, the
    selection per round with the flags of that moment"""
    from .matcher import ORBmatcher
    nb = stream["neighbours"]
    live = [k for k, kf in enumerate(nb) if kf is not None]
    tb = ORBmatcher(0.6, False, extractor=ex).TriangulationBatch(stream["kf1"], [nb[k] for k in live])
    slot = {k: j for j, k in enumerate(live)}

    def select(k, has1, has2):
        kf1, kf2 = dict(stream["kf1"], has_map_point=has1), dict(nb[k], has_map_point=has2)
        return tb.select(slot[k], kf1, kf2, stream["F12"][k], stream["epipole"][k])[1]
    return select, tb


def create_new_map_points_rounds(ex, streams):
    """The neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:378-679) for S streams at once.  Within one
    keyframe the neighbours are sequential -- a point created for neighbour k sets GetMapPoint(idx1) of the current keyframe, and
    SearchForTriangulation of neighbour k + 1 skips that feature -- so round k does, in order: the selection for neighbour k of
    every stream that still has one, ONE create_new_map_points_batch call for all of them, and has_map_point set for both features
    of every accepted match before round k + 1.

    streams: [{"kf1": keyframe with has_map_point, "neighbours": [keyframe with has_map_point, or None], ...}].  A neighbour the
    baseline / median-depth gate of :403-420 rejects is None: it is skipped, as `continue` does.  The selection is
    stream["select"](k, has1, has2) -> matches12 [KF1.N] when given; otherwise orbx_triangulation_batch_select through
    ORBmatcher.TriangulationBatch with stream["F12"][k] and stream["epipole"][k].  ComputeF12 needs cv::Mat::inv and stays with the
    caller, like the gate and the epipole: the library starts where the reference holds F12.
    Returns per stream the accepted [(k, idx1, idx2, point float32 [3])] in creation order.  The caller's flags are not modified;
    AddObservation, Map::AddMapPoint and the refresh of the new points (distinctive_descriptors_batch,
    update_normal_and_depth_batch) follow on the caller's side."""
    S = len(streams)
    state, closers = [], []
    try:
        for s in streams:
            sel = s.get("select")
            if sel is None:
                sel, tb = _default_select(ex, s)
                closers.append(tb)
            has1 = np.array(s["kf1"]["has_map_point"], np.uint8)
            has2 = [None if kf is None else np.array(kf["has_map_point"], np.uint8) for kf in s["neighbours"]]
            state.append((sel, has1, has2))
        created = [[] for _ in range(S)]
        for k in range(max((len(s["neighbours"]) for s in streams), default=0)):
            who, problems = [], []
            for j, s in enumerate(streams):
                if k >= len(s["neighbours"]) or s["neighbours"][k] is None:
                    continue
                sel, has1, has2 = state[j]
                pairs = matched_pairs(sel(k, has1.copy(), has2[k].copy()))
                who.append(j)
                problems.append({"kf1": s["kf1"], "kf2": s["neighbours"][k], "matches": pairs})
            if not problems:
                continue
            for j, p, (status, points) in zip(who, problems, create_new_map_points_batch(ex, problems)):
                _, has1, has2 = state[j]
                for m in np.nonzero(np.isin(status, ACCEPTED))[0]:
                    i1, i2 = int(p["matches"][m, 0]), int(p["matches"][m, 1])
                    has1[i1] = 1
                    has2[k][i2] = 1
                    created[j].append((k, i1, i2, points[m].copy()))
        return created
    finally:
        for tb in closers:
            tb.close()


def local_bundle_adjustment_rounds(ex, streams, refresh=None):
    """Optimizer::LocalBundleAdjustment for the keyframe each of B streams has just processed: ONE
    optimizer.local_bundle_adjustment_batch call for all streams, then -- as src/Optimizer.cc:1028 does per point -- ONE
    mappoint.update_normal_and_depth_batch call over the moved points of all streams.

    streams: dicts with the problem keys of optimizer.local_bundle_adjustment_batch (nlocal, Tcw, local_fixed, camera, bf, world,
    obs_begin, obs_kf, obs, inv_sigma2, second_round) and, for the refresh, ref_kf [npoints] (index of each point's reference
    keyframe in the keyframe list) and ref_level [npoints] (the octave of the point's keypoint in it).  A stream whose stop flag
    is set on entry is passed as None and is skipped (src/Optimizer.cc:886-888).  refresh=False skips the second call (it needs
    a device handle).  Returns per stream None or a dict: Tcw [nlocal, 16], world [npoints, 3], erase [nobs], info, and with the
    refresh normal [npoints, 3], min_distance, max_distance.  The refresh reads the optimised poses and points and leaves the
    erased observations out, as the map would hold them after the erase list is applied."""
    from . import mappoint, optimizer
    who = [j for j, s in enumerate(streams) if s is not None]
    out = [None] * len(streams)
    got = optimizer.local_bundle_adjustment_batch(ex, [streams[j] for j in who])
    for j, (T, w, e, info) in zip(who, got):
        out[j] = {"Tcw": T, "world": w, "erase": e, "info": info}
    if refresh is None:
        refresh = all("ref_kf" in streams[j] for j in who) and bool(who)
    if not refresh:
        return out
    begin, pos, centers, refc, level, counts = [0], [], [], [], [], []
    for j in who:
        s, r = streams[j], out[j]
        T = np.array(np.asarray(s["Tcw"], np.float32).reshape(-1, 4, 4))
        T[:s["nlocal"]] = r["Tcw"].reshape(-1, 4, 4)
        Ow = -np.einsum("kji,kj->ki", T[:, :3, :3], T[:, :3, 3])        # GetCameraCenter: -R^T t, in float as SetPose computes it
        ob = np.asarray(s["obs_begin"], np.int64)
        kf = np.asarray(s["obs_kf"], np.int64)
        for p in range(len(ob) - 1):
            live = np.arange(ob[p], ob[p + 1])[r["erase"][ob[p]:ob[p + 1]] == 0]
            centers.append(Ow[kf[live]])
            begin.append(begin[-1] + len(live))
        pos.append(r["world"]); refc.append(Ow[np.asarray(s["ref_kf"], np.int64)]); level.append(np.asarray(s["ref_level"], np.int32))
        counts.append(len(ob) - 1)
    if begin[-1] == 0 and not sum(counts):
        return out
    normal, dmin, dmax = mappoint.update_normal_and_depth_batch(
        ex, np.array(begin, np.int32), np.concatenate(pos).reshape(-1, 3), np.concatenate(centers).reshape(-1, 3) if centers else np.zeros((0, 3)),
        np.concatenate(refc).reshape(-1, 3), np.concatenate(level))
    at = 0
    for j, n in zip(who, counts):
        out[j].update(normal=normal[at:at + n], min_distance=dmin[at:at + n], max_distance=dmax[at:at + n])
        at += n
    return out
