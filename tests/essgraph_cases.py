"""The scene list of tests/test_essgraph_cpu.py and tests/test_essgraph_gpu.py with the model's answers, computed once per
process: both files run the same problems and compare with the same function."""
import functools

import numpy as np

import essgraph_model as em
import essgraph_scenes as sc
from orb_slam2_detailed_comments_amd import optimizer

SMALL = dict(rot_noise=1e-4, t_noise=1e-3, s_noise=1e-7)   # inside d > 1 - 1e-5 and |log s| < 1e-5


@functools.lru_cache(maxsize=None)
def scenes():
    """What the implementation branches on, not the workload: the 64 chains over a vertex's edges, over the edges and over the
    columns; 256 lanes over the items of a phase; the number of rounds; fill; the four branches of Sim3::log."""
    s = {}
    s["two"] = sc.make(1, 2, [(1, 0, 0)])
    s["chain3"] = sc.make(2, 3, sc.path_edges(3), npoints=1, ref=[0])                      # one point, on the fixed vertex
    s["path9"] = sc.make(3, 9, sc.path_edges(9), npoints=5)
    s["path9_fix_scale"] = sc.make(3, 9, sc.path_edges(9), fix_scale=True, npoints=5)
    s["path9_small"] = sc.make(4, 9, sc.path_edges(9), **SMALL)
    s["path9_small_rot"] = sc.make(5, 9, sc.path_edges(9), rot_noise=1e-4, t_noise=1e-3, s_noise=0.02)
    s["path9_fix_scale_small"] = sc.make(6, 9, sc.path_edges(9), fix_scale=True, rot_noise=1e-4, t_noise=1e-3)
    # (seeds whose optimisation ends after 5 / 6 iterations: the model's run stays at a second or two)
    s["path65"] = sc.make(33, 65, sc.path_edges(65), rot_noise=0.005, t_noise=0.02, s_noise=0.005)
    s["path257"] = sc.make(31, 257, sc.path_edges(257), rot_noise=0.005, t_noise=0.02, s_noise=0.005, npoints=257)
    for n in (63, 64, 65, 129):
        s["star%d" % n] = sc.star(10 + n, n, rot_noise=0.01, t_noise=0.02, s_noise=0.01)
    s["cycle_chord"] = sc.cycle_chord(20)
    s["parallel"] = sc.make(21, 3, [(1, 0, 1), (1, 0, 0), (2, 1, 1), (2, 1, 0)])
    s["isolated"] = sc.make(22, 5, [(1, 0, 0), (2, 1, 0)], fixed=(0, 4), npoints=3, ref=[3, 4, 1])   # 3: free, 4: fixed, no edge
    s["no_fixed"] = sc.make(23, 4, [(1, 0, 0), (2, 1, 0), (3, 2, 0), (3, 0, 1)], fixed=())
    s["two_fixed"] = sc.make(24, 4, [(1, 0, 0), (2, 1, 0), (3, 2, 0), (3, 0, 0)], fixed=(0, 3))        # (3, 0): both fixed
    s["consistent"] = sc.consistent()
    s["loop"] = sc.loop()
    s["empty"] = dict(Scw=np.zeros((0, 8)), fixed=np.zeros(0, np.uint8), edges=np.zeros((0, 3), np.int32), fix_scale=False,
                      world=np.zeros((0, 3), np.float32), ref=np.zeros(0, np.int32))
    return s


_MODELS = {}


def model(p):
    """the model's answer and trace for a scene object, computed once"""
    k = id(p)
    if k not in _MODELS:
        tr = {}
        _MODELS[k] = (em.run(p, tr), tr, p)
    return _MODELS[k][0], _MODELS[k][1]


def run(ex, problems, per_call=16):
    out = []
    for i in range(0, len(problems), per_call):
        out += optimizer.optimize_essential_graph_batch(ex, list(problems[i:i + per_call]))
    return out


def u64(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


def u32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def assert_same(a, b, what):
    """two library answers, bit for bit"""
    assert np.array_equal(u64(a[0]), u64(b[0])), what + ": Siw"
    assert np.array_equal(u32(a[1]), u32(b[1])), what + ": Tiw"
    assert np.array_equal(u32(a[2]), u32(b[2])), what + ": points"
    assert a[3].tobytes() == b[3].tobytes(), what + ": record"


def assert_equal(got, mo, what):
    S, T, w, info = got
    for k in ("iters", "nactive", "nfailed", "nrounds", "nlblocks"):
        assert int(info[k]) == int(mo[k]), "%s: %s %d, model %d" % (what, k, int(info[k]), int(mo[k]))
    assert np.array_equal(u64(info["chi2"]), u64(mo["chi2"])), what + ": chi2"
    assert np.array_equal(u64(info["lambda"]), u64(mo["lambda"])), what + ": lambda"
    assert np.array_equal(u64(S), u64(mo["Siw"])), what + ": Siw"
    assert np.array_equal(u32(T), u32(mo["Tiw"])), what + ": Tiw"
    assert np.array_equal(u32(w), u32(mo["world"])), what + ": points"


def assert_all(ex, named):
    names = list(named)
    got = run(ex, [named[n] for n in names])
    for n, g in zip(names, got):
        assert_equal(g, model(named[n])[0], str(n))
    return dict(zip(names, got))
