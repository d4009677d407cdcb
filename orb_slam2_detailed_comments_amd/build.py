"""Builds liborbx.so (HIP kernels + C ABI) for gfx950 with hipcc, in-tree.

hipcc cross-compiles without a GPU; the resulting .so travels to the GPU box with the repo snapshot.
-ffp-contract=off: no implicit FMA in host or device code (every fused operation is explicit).
"""
from __future__ import annotations
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "liborbx.so")
# the ONE list of what the library is built from: the build, the rebuild check, kernels_hash() and tools/build_variant.sh use it
SOURCES = ["orbx_kernels.hip", "orbx_api.cpp", "orbx_extract.cpp", "orbx_pyramid.cpp", "orbx_match.cpp", "orbx_tracking.cpp",
           "orbx_map_batches.cpp", "orbx_bow.cpp", "orbx_geometry.cpp", "orbx_policies.cpp", "orbx_kfdb.cpp", "orbx_track_pack.cpp",
           "orbx_mappoint.cpp", "orbx_pose.cpp", "orbx_sim3opt.cpp", "orbx_sim3.cpp", "orbx_pnp.cpp", "orbx_init.cpp", "orbx_recon.cpp",
           "orbx_newpoints.cpp", "orbx_sim3search.cpp", "orbx_localba.cpp", "orbx_essgraph.cpp"]
HEADERS = ["orbx_device.h", "orbx_inplace.h", "orbx_fast_net.h", "orbx_internal.h", "orbx_launch.h", "orbx_sincos.h", "orbx_track.h",
           "orbx_mappoint.h", "orbx_lm.h", "orbx_pose.h", "orbx_sim3opt.h", "orbx_localba.h", "orbx_essgraph.h", "orbx_ransac.h", "orbx_sim3.h", "orbx_pnp.h", "orbx_init.h", "orbx_recon.h", "orbx_newpoints.h", "orbx_sim3search.h", "orbx_handle.h", "orbx_gate.h", os.path.join("..", "..", "include", "orbx.h"),
           os.path.join("..", "..", "include", "orbx_pattern_data.h"), os.path.join("..", "..", "include", "orbx_rect_digest.h")]


def kernels_hash():
    """identity of the device code AND of what decides its launch geometry (kernel source, device headers, the launch plans of
    orbx_extract.cpp): every file of SOURCES and HEADERS, so none can be missed.  profiles/*_traffic.json and *_sq.json carry it,
    so counters taken on other kernels or other launch plans read as 'not measured' in bench.py instead of as stale numbers"""
    import hashlib
    h = hashlib.sha256()
    for f in SOURCES + HEADERS:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    return h.hexdigest()[:16]


def hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the ORB front-end has no non-HIP build")


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS)


def build(force=False, verbose=False, extra=(), out=None):
    """out: build a variant library there (always; extra carries its flags) instead of the package's own"""
    if out is None and not force and not needs_build():
        return LIB
    lib = out or LIB
    os.makedirs(os.path.dirname(os.path.abspath(lib)), exist_ok=True)
    cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-x", "hip",
           "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value",
           *extra, *[os.path.join(CSRC, s) for s in SOURCES], "-o", lib]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True,
                extra=("-Rpass-analysis=kernel-resource-usage",) if "--usage" in sys.argv else ()))
