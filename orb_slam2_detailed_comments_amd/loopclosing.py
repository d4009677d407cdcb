"""LoopClosing::CorrectLoop's pose graph (Optimizer::OptimizeEssentialGraph, src/Optimizer.cc:1050-1358) from plain arrays: the
edge selection of steps 3 and 4 (:1139-1291) and the Sim3 of a keyframe that has no CorrectedSim3 (:1109-1113).  The
optimisation itself is optimizer.optimize_essential_graph_batch.

Keyframes are indices 0..n-1 in the order of Map::GetAllKeyFrames, bad ones included (they get no vertex in the reference and
no edge here); `ids` carries mnId where that order is not the order of the indices."""
from __future__ import annotations
import numpy as np

MIN_FEAT = 100   # minFeat, :1084


def _weight(weights, i, j):
    """KeyFrame::GetWeight: 0 where the pair is not connected"""
    if callable(weights):
        return int(weights(i, j))
    if isinstance(weights, dict):
        return int(weights.get((i, j), weights.get((j, i), 0)))
    return int(weights[i][j])


def essential_graph_edges(n, cur, loop, loop_connections, weights, parents, loop_edges, covisibles, children=None, bad=None,
                          ids=None, min_feat=MIN_FEAT):
    """The edges of OptimizeEssentialGraph as int32 [ne, 3] rows (i, j, kind), vertex 0 = i and vertex 1 = j of the EdgeSim3, in
    the order the reference adds them.
    Step 3 (:1139-1177), kind 1: loop_connections = [(i, [j, ...]), ...] in the order LoopConnections is walked; a pair is kept
    when it is (cur, loop) or GetWeight >= min_feat, and enters sInsertedEdges.
    Step 4 (:1181-1291), kind 0, per keyframe i: the spanning-tree edge to parents[i] (-1: none); the loop edges loop_edges[i] with
    a smaller mnId; the covisibles covisibles[i] (GetVectorCovisibleKeyFrames order: weight descending) with weight >= min_feat
    that are not the parent, not a child, not a loop edge, not bad, have a smaller mnId and are not in sInsertedEdges.
    sInsertedEdges guards only these covisibility edges, so a loop-connection edge and a spanning-tree edge can join one pair: the
    graph then has two parallel edges, as in the reference.
    A bad keyframe has no vertex (the reference dereferences optimizer.vertex(id) of one, :1166): every edge with a bad end is left
    out, as compat/Optimizer_essentialgraph.inl does.
    weights: a callable (i, j), a dict {(i, j): w} or a square array.  children[i]: KeyFrame::hasChild, by default the keyframes
    whose parent is i."""
    bad = np.zeros(n, bool) if bad is None else np.asarray(bad, bool)
    ids = np.arange(n) if ids is None else np.asarray(ids)
    parents = np.asarray(parents, np.int64)
    if children is None:
        children = [set() for _ in range(n)]
        for c in range(n):
            if parents[c] >= 0:
                children[int(parents[c])].add(c)
    out, inserted = [], set()
    for i, conns in loop_connections:
        for j in conns:
            if (i != cur or j != loop) and _weight(weights, i, j) < min_feat:
                continue
            if bad[i] or bad[j]:
                continue
            out.append((i, j, 1))
            inserted.add((min(ids[i], ids[j]), max(ids[i], ids[j])))
    for i in range(n):
        if bad[i]:
            continue
        p = int(parents[i])
        if p >= 0 and not bad[p]:
            out.append((i, p, 0))
        le = list(loop_edges[i])
        for l in le:
            if ids[l] < ids[i] and not bad[l]:
                out.append((i, l, 0))
        for k in covisibles[i]:
            if _weight(weights, i, k) < min_feat:
                continue
            if k == p or k in children[i] or k in le:
                continue
            if bad[k] or not ids[k] < ids[i]:
                continue
            if (min(ids[i], ids[k]), max(ids[i], ids[k])) in inserted:
                continue
            out.append((i, k, 0))
    return np.array(out, np.int32).reshape(-1, 3)


def sim3_from_Tcw(Tcw):
    """g2o::Sim3(toMatrix3d(Rcw), toVector3d(tcw), 1.0) (:1109-1111) as the 8 doubles of a problem's Scw row: the floats widened,
    Eigen's Quaterniond(Matrix3d) (its trace > 0 branch and the three others), nothing normalised"""
    M = np.asarray(Tcw, np.float32).reshape(4, 4).astype(np.float64)
    m = M[:3, :3]
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        x, y, z = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q = [0.0, 0.0, 0.0]
        q[i] = 0.5 * t
        t = 0.5 / t
        w = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
        x, y, z = q
    return np.array([x, y, z, w, M[0, 3], M[1, 3], M[2, 3], 1.0], np.float64)
