"""compat/Optimizer_sim3.inl (the body for Optimizer::OptimizeSim3), syntax only: the stand-ins of tests/compat_sim3 have no
mvInvLevelSigma2, no g2o::Sim3 and no Eigen, so tests/compat_sim3opt/check.cpp declares the members the body touches, over the cv
stand-in of tests/compat_runtime.  Needs neither the library nor a GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compat_sim3opt_body_compiles_without_warnings():
    assert shutil.which("g++")
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "tests", "compat_runtime"),
           "-I" + os.path.join(ROOT, "compat"), "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "compat_sim3opt", "check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr[-4000:]
