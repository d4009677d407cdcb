"""compat/Optimizer_essentialgraph.inl (the body of Optimizer::OptimizeEssentialGraph from :1090 on) through the stand-ins of
tests/compat_essgraph/: built with -Wall -Werror, one scene run through the fragment on a host-only handle; the poses and the
points equal the Python path (loopclosing.essential_graph_edges, loopclosing.sim3_from_Tcw,
optimizer.optimize_essential_graph_batch) bit for bit, and so tests/essgraph_model.py.  The fragment walks std::map and std::set
of KeyFrame *, ascending address, which is ascending keyframe index in the harness.  Needs no GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import essgraph_model as em
import essgraph_scenes as sc
from orb_slam2_detailed_comments_amd import ORBextractor, _capi, loopclosing, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "compat_essgraph")
LIBDIR = os.path.dirname(_capi.LIB_PATH)


def build_cmd(out):
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", "-ffp-contract=off", "-I" + HERE,
           "-I" + os.path.join(ROOT, "tests", "compat_runtime"), "-I" + os.path.join(ROOT, "compat"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "harness.cpp")]
    if out is None:
        return cmd + ["-fsyntax-only"]
    return cmd + ["-shared", "-fPIC", "-L" + LIBDIR, "-lorbx", "-Wl,-rpath," + LIBDIR, "-o", out]


def test_compat_essgraph_syntax():
    assert shutil.which("g++")
    p = subprocess.run(build_cmd(None), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]


def scene():
    """14 keyframes on a drifting arc: keyframe 7 is bad, 6's parent is 4 (also covisible with weight 100), an earlier loop edge
    9 - 3, the last three carry CorrectedSim3 / NonCorrectedSim3, pCurKF = 13 closes on pLoopKF = 0"""
    n, cur, loop = 14, 13, 0
    lp = sc.loop(seed=9, n=n, ncorr=3, npoints=0)
    S = lp["non_corrected"]                                    # the tracked poses, scale 1
    Tcw = np.zeros((n, 16), np.float32)
    for k in range(n):
        R = np.array(em._R_from_quat(S[k].reshape(8, 1))).reshape(3, 3)
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = S[k, 4:7]
        Tcw[k] = T.astype(np.float32).reshape(16)
    bad = np.zeros(n, np.uint8); bad[7] = 1
    parents = np.arange(-1, n - 1); parents[6] = 4; parents[8] = 6
    W = np.zeros((n, n), np.int32)
    for i in range(n):
        for j in range(i):
            W[i, j] = W[j, i] = {1: 260 - 3 * i, 2: 100 + (i % 3) * 15, 3: 99 + (i % 2) * 3}.get(i - j, 0)
    W[13, 0] = W[0, 13] = 70; W[13, 1] = W[1, 13] = 130; W[12, 0] = W[0, 12] = 40; W[9, 3] = W[3, 9] = 120
    loop_edges = [(9, 3), (3, 9)]
    conns = [(0, 12), (0, 13), (1, 13), (12, 0), (12, 13), (13, 0), (13, 1), (13, 12)]
    has_c = np.zeros(n, np.uint8); has_c[11:] = 1
    rng = np.random.default_rng(4)
    npts = 40
    world = rng.normal(0, 4, (npts, 3)).astype(np.float32)
    ref_kf = rng.integers(0, n, npts).astype(np.int32); ref_kf[3] = 7; ref_kf[4] = 0
    pt_bad = np.zeros(npts, np.uint8); pt_bad[::9] = 1
    by_cur = np.zeros(npts, np.uint8); by_cur[5::7] = 1
    cref = rng.integers(11, n, npts).astype(np.int32)
    return dict(n=n, cur=cur, loop=loop, Tcw=Tcw, bad=bad, parents=parents.astype(np.int32), W=W, loop_edges=loop_edges, conns=conns,
                has_c=has_c, corrected=np.ascontiguousarray(lp["Scw"]), has_nc=has_c.copy(), non_corrected=np.ascontiguousarray(S),
                world=world, ref_kf=ref_kf, pt_bad=pt_bad, by_cur=by_cur, cref=cref)


def python_path(host, s, fix_scale):
    n = s["n"]
    vertex = np.full(n, -1, np.int32)
    vertex[s["bad"] == 0] = np.arange(int((s["bad"] == 0).sum()))
    keep = np.nonzero(s["bad"] == 0)[0]
    Scw = np.stack([s["corrected"][k] if s["has_c"][k] else loopclosing.sim3_from_Tcw(s["Tcw"][k]) for k in keep])
    le = [[] for _ in range(n)]
    for i, j in s["loop_edges"]:
        le[i].append(j)
    conns = {}
    for i, j in s["conns"]:
        conns.setdefault(i, []).append(j)
    cov = [sorted((j for j in range(n) if j != i and s["W"][i][j] > 0), key=lambda j: -s["W"][i][j]) for i in range(n)]
    E = loopclosing.essential_graph_edges(n, s["cur"], s["loop"], sorted((i, sorted(js)) for i, js in conns.items()), s["W"],
                                          s["parents"], le, cov, bad=s["bad"])
    E = np.stack([vertex[E[:, 0]], vertex[E[:, 1]], E[:, 2]], axis=1).astype(np.int32)
    assert (E[:, :2] >= 0).all()
    ref = np.where(s["by_cur"] == 1, s["cref"], s["ref_kf"])
    ref = np.where(s["pt_bad"] == 1, -1, vertex[ref]).astype(np.int32)
    fixed = np.zeros(len(keep), np.uint8); fixed[vertex[s["loop"]]] = 1
    p = dict(Scw=Scw, fixed=fixed, non_corrected=s["non_corrected"][keep], has_non_corrected=s["has_nc"][keep], edges=E,
             fix_scale=fix_scale, world=s["world"], ref=ref)
    (Siw, Tiw, world, info), = optimizer.optimize_essential_graph_batch(host, [p])
    return keep, E, ref, Tiw, world, info


def run_fragment(L, s, fix_scale):
    n, npts = s["n"], len(s["world"])
    T, w, info = np.full((n, 16), 7.5, np.float32), np.full((npts, 3), 7.5, np.float32), np.zeros(4, np.int32)
    le, cn = np.array(s["loop_edges"], np.int32).reshape(-1, 2), np.array(s["conns"], np.int32).reshape(-1, 2)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    L.eg_compat_run.restype = C.c_int
    L.eg_compat_run.argtypes = ([C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 4
                                + [C.c_void_p] * 8)
    Wc = np.ascontiguousarray(s["W"], np.int32)
    rc = L.eg_compat_run(n, ptr(s["Tcw"]), ptr(s["bad"]), ptr(s["parents"]), ptr(Wc), len(le), ptr(le), len(cn), ptr(cn), ptr(s["has_c"]),
                         ptr(s["corrected"]), ptr(s["has_nc"]), ptr(s["non_corrected"]), s["cur"], s["loop"], int(fix_scale), npts,
                         ptr(s["world"]), ptr(s["ref_kf"]), ptr(s["pt_bad"]), ptr(s["by_cur"]), ptr(s["cref"]), ptr(T), ptr(w), ptr(info))
    return rc, T, w, info


def test_fragment_equals_the_python_path(built_lib, tmp_path):
    so = str(tmp_path / "compat_essgraph.so")
    b = subprocess.run(build_cmd(so), capture_output=True, text=True, timeout=600)
    assert b.returncode == 0 and "warning" not in b.stderr, b.stderr[-4000:]
    L = C.CDLL(so)
    host = ORBextractor(1000, 1.2, 8, 20, 7, device=-2)
    try:
        s = scene()
        for fix_scale in (False, True):
            keep, E, ref, Tiw, world, info = python_path(host, s, fix_scale)
            rows = [tuple(r) for r in E]
            assert int(info["iters"]) >= 1 and info["chi2"][1] < info["chi2"][0] and len(E) > 20
            assert sum(1 for r in rows if r[2] == 1) == 5            # (0, 13) and (1, 13) ... by weight or as (cur, loop); 12 - 0 is too weak
            rc, Tf, wf, finfo = run_fragment(L, s, fix_scale)
            assert rc == 0
            assert np.array_equal(Tf[keep].view(np.uint32), Tiw.view(np.uint32))
            assert np.array_equal(Tf[7], s["Tcw"][7])                  # the bad keyframe keeps its pose
            assert np.array_equal(wf.view(np.uint32), world.view(np.uint32))
            live = int((ref >= 0).sum())
            assert list(finfo) == [len(keep), live, live, 2]
            assert ref[3] == -1 and np.array_equal(wf[3], s["world"][3])   # its reference keyframe is bad
    finally:
        host.close()
