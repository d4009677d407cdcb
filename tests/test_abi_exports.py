"""The library exports exactly the functions include/orbx.h declares.  `-shared` links happily with a unit missing from
build.py's SOURCES (the entry points it held just stay undefined until somebody loads the library and calls one): this
test names the missing, or the stray, entry points instead."""
import os
import re
import shutil
import subprocess

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orbx.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return set(re.findall(r"\b(orbx_[a-z0-9_]+)\(", src))


def _exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        f = line.split()
        if len(f) >= 2 and f[-2] == "T" and f[-1].startswith("orbx_"):   # C++-mangled names start with _Z
            names.add(f[-1])
    return names


def test_exports_are_the_declared_entry_points(built_lib):
    if not shutil.which("nm"):
        pytest.skip("nm not installed")
    declared, exported = _declared(), _exported(built_lib)
    assert declared, "no declaration found in include/orbx.h"
    assert exported == declared, (f"declared, not exported: {sorted(declared - exported)}; "
                                  f"exported, not declared: {sorted(exported - declared)}")
