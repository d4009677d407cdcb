"""The stand-in harness of tests/compat_mappoint/ (MapPoint / KeyFrame stand-ins, the two MapPoint functions as single calls,
compat/MapPoint_batch.inl) for tests/test_mappoint_batch_cpu.py and tests/test_compat_mappoint.py: how it is built, a ctypes
wrapper, and the scene both tests play."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "compat_mappoint")
LIBDIR = os.path.join(ROOT, "orb_slam2_detailed_comments_amd", "lib")
LEVELS, FACTOR = 8, 1.2


def build_cmd(out, syntax_only=False):
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-O1", "-ffp-contract=off", "-I" + HERE,
           "-I" + os.path.join(ROOT, "tests", "compat_runtime"), "-I" + os.path.join(ROOT, "compat"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "harness.cpp")]
    if syntax_only:
        return cmd + ["-fsyntax-only"]
    return cmd + [os.path.join(HERE, "map_model.cpp"), "-shared", "-fPIC", "-L" + LIBDIR, "-lorbx", "-Wl,-rpath," + LIBDIR, "-o", out]


def build(out):
    p = subprocess.run(build_cmd(out), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]
    return Map(out)


class Map:
    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.mpt_error.restype = C.c_char_p
        self.call("mpt_reset")
        self.kf_desc = []

    def call(self, name, *args):
        conv = [a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a for a in args]
        assert getattr(self.L, name)(*conv) == 0, self.L.mpt_error().decode()

    def keyframe(self, desc, octave, Ow):
        out = np.zeros(1, np.int32)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.call("mpt_add_keyframe", len(desc), desc, np.ascontiguousarray(octave, np.int32), np.ascontiguousarray(Ow, np.float32),
                  LEVELS, C.c_float(FACTOR), out)
        self.kf_desc.append(desc)
        return int(out[0])

    def point(self, pos, ref_kf, desc, normal, dmin, dmax):
        out = np.zeros(1, np.int32)
        self.call("mpt_add_point", np.ascontiguousarray(pos, np.float32), int(ref_kf), np.ascontiguousarray(desc, np.uint8),
                  np.ascontiguousarray(normal, np.float32), C.c_float(dmin), C.c_float(dmax), out)
        return int(out[0])

    def restore(self, pts):
        for p, P in enumerate(pts):
            self.call("mpt_restore", p, np.ascontiguousarray(P["desc"], np.uint8), np.ascontiguousarray(P["normal"], np.float32),
                      C.c_float(P["dmin"]), C.c_float(P["dmax"]))

    def obs(self, mp, cap=512):
        kf, idx, n = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(1, np.int32)
        self.call("mpt_obs", int(mp), kf, idx, cap, n)
        assert n[0] <= cap
        return list(zip(kf[:n[0]].tolist(), idx[:n[0]].tolist()))

    def state(self, mp):
        d, out = np.zeros(32, np.uint8), np.zeros(5, np.float32)
        self.call("mpt_state", int(mp), d, out)
        return d, out

    def states(self, n):
        s = [self.state(p) for p in range(n)]
        return np.stack([a for a, _ in s]), np.stack([b for _, b in s])


def play_scene(M, seed=11, npoints=300, nkf=12, nslots=320):
    """about 300 points over 12 keyframes with random float positions and centres: a bad point, an unobserved point, a bad
    keyframe, a point all of whose keyframes are bad.  Returns what the Python model needs: per point (pos, ref_kf, initial
    descriptor / normal / distances, bad), per keyframe (descriptors, octaves, centre, bad), and the list to refresh (with a
    duplicated entry and a NULL)."""
    import mappoint_model as mm
    rng = np.random.default_rng(seed)
    M.call("mpt_reset"); M.kf_desc = []
    protos = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    kfs = []
    for k in range(nkf):
        desc = np.stack([mm.flip(rng, protos[rng.integers(0, 6)], int(rng.integers(0, 5))) for _ in range(nslots)])
        octv = rng.integers(0, LEVELS, nslots).astype(np.int32)
        octv[0], octv[1] = 0, LEVELS - 1
        Ow = rng.normal(0, 2.0, 3).astype(np.float32)
        M.keyframe(desc, octv, Ow)
        kfs.append(dict(desc=desc, octave=octv, Ow=Ow, bad=False))
    pts = []
    for p in range(npoints):
        n = int(rng.integers(1, nkf + 1))
        if p == 5:
            n = 0                                                    # unobserved
        which = rng.permutation(nkf)[:n]
        if p == 9:
            which = np.array([3])                                    # observed by the bad keyframe alone
        ref = int(which[0]) if len(which) else 0
        pos = (rng.normal(0, 2.0, 3) + np.array([0, 0, 6.0])).astype(np.float32)
        d0 = rng.integers(0, 256, 32, dtype=np.uint8)
        n0 = rng.normal(size=3).astype(np.float32)
        dmin, dmax = np.float32(rng.uniform(0.1, 1)), np.float32(rng.uniform(2, 9))
        M.point(pos, ref, d0, n0, dmin, dmax)
        for k in which:                                              # insertion order is not the map's order
            M.call("mpt_observe", p, int(k), p)
        pts.append(dict(pos=pos, ref=ref, desc=d0, normal=n0, dmin=dmin, dmax=dmax, bad=False))
    M.call("mpt_set_bad", 7); pts[7]["bad"] = True
    M.call("mpt_kf_set_bad", 3); kfs[3]["bad"] = True
    order = list(range(npoints))
    order.insert(40, 12)                                             # a point that appears twice
    order.insert(100, -1)                                            # a NULL entry
    return pts, kfs, np.array(order, np.int32)


def model_scene(M, pts, kfs):
    """what the two functions must leave behind, from tests/mappoint_model.py fed the map's own order (mpt_obs)"""
    import mappoint_model as mm
    scale = mm.scale_factors(LEVELS, FACTOR)
    descs, outs = [], []
    for p, P in enumerate(pts):
        obs = [] if P["bad"] else M.obs(p)
        d, nrm, dmin, dmax = P["desc"], P["normal"], P["dmin"], P["dmax"]
        rows = [kfs[k]["desc"][i] for k, i in obs if not kfs[k]["bad"]]
        if rows:
            d = rows[mm.distinct_one(np.stack(rows))[0]]
        if obs:
            level = kfs[P["ref"]]["octave"][dict(obs)[P["ref"]]]
            nrm, dmin, dmax = mm.normal_depth_one(P["pos"], np.stack([kfs[k]["Ow"] for k, _ in obs]), kfs[P["ref"]]["Ow"],
                                                  scale[level], scale[LEVELS - 1])
        descs.append(d); outs.append(np.concatenate([nrm, [dmin, dmax]]).astype(np.float32))
    return np.stack(descs), np.stack(outs)
