"""Compiles the reference's own DBoW2 and KeyFrameDatabase sources, unmodified and straight from the reference tree, behind the
stand-in headers of this directory and the C ABI of harness.cpp, into oracle/_ref/ (kept out of git):

    libref_dbow2_strict.so   g++ -O3 -ffp-contract=off    what fp_mode = FP_STRICT stands for
    libref_dbow2_fma.so      g++ -O3 -mfma                what fp_mode = FP_GCC_FMA stands for (GCC contracts a * b + c where its
                                                          default -ffp-contract=fast allows it; an explicit ISA flag, not
                                                          -march=native, because the binaries travel to other machines)
    BUILD_INFO.txt           compiler version, flags, source list

The reference tree is read from $ORB_SLAM2_REFERENCE, by default the directory `reference` beside the repository.  Nothing of
it is copied: the compiler reads the sources where they are."""
import os
import shutil
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(os.path.dirname(HERE), "_ref")
SOURCES = ["Thirdparty/DBoW2/DBoW2/BowVector.cpp", "Thirdparty/DBoW2/DBoW2/ScoringObject.cpp",
           "Thirdparty/DBoW2/DBoW2/FeatureVector.cpp", "Thirdparty/DBoW2/DBoW2/FORB.cpp", "Thirdparty/DBoW2/DUtils/Random.cpp",
           "Thirdparty/DBoW2/DUtils/Timestamp.cpp", "src/KeyFrameDatabase.cc"]
VARIANTS = {"strict": ["-O3", "-ffp-contract=off"], "fma": ["-O3", "-mfma"]}


def reference_dir():
    return os.environ.get("ORB_SLAM2_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))


def reference_present():
    ref = reference_dir()
    return all(os.path.isfile(os.path.join(ref, s)) for s in SOURCES)


def lib_path(variant):
    return os.path.join(OUT, "libref_dbow2_%s.so" % variant)


def built():
    return all(os.path.isfile(lib_path(v)) for v in VARIANTS)


def command(variant, out):
    ref = reference_dir()
    # -include: the stand-ins define the include guards of the reference's KeyFrame.h / Frame.h before KeyFrameDatabase.h
    # includes its siblings by quoted name; -I HERE first: <opencv2/core/core.hpp> is the stand-in
    return (["g++", "-std=c++11", "-w", "-shared", "-fPIC"] + VARIANTS[variant] +
            ["-I" + HERE, "-I" + ref, "-I" + os.path.join(ref, "include"),
             "-include", os.path.join(HERE, "KeyFrame.h"), "-include", os.path.join(HERE, "Frame.h")] +
            [os.path.join(ref, s) for s in SOURCES] + [os.path.join(HERE, "harness.cpp"), "-lpthread", "-o", out])


def build(force=False):
    """Returns the seconds spent compiling (0.0 when everything is up to date)."""
    if not reference_present():
        raise FileNotFoundError("reference tree not found at %s (set ORB_SLAM2_REFERENCE)" % reference_dir())
    if shutil.which("g++") is None:
        raise RuntimeError("g++ not found")
    os.makedirs(OUT, exist_ok=True)
    mine = [os.path.join(HERE, f) for f in ("harness.cpp", "KeyFrame.h", "Frame.h", "build_ref.py", "opencv2/core/core.hpp")]
    deps = mine + [os.path.join(reference_dir(), s) for s in SOURCES]
    newest = max(os.path.getmtime(d) for d in deps)
    t0 = time.time()
    jobs = []
    for variant in VARIANTS:            # the two builds side by side
        so = lib_path(variant)
        if not force and os.path.isfile(so) and os.path.getmtime(so) >= newest:
            continue
        tmp = so + ".tmp%d" % os.getpid()
        jobs.append((variant, so, tmp, subprocess.Popen(command(variant, tmp), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)))
    did = bool(jobs)
    errors = []
    for variant, so, tmp, p in jobs:
        err = p.communicate()[1]
        if p.returncode != 0:
            errors.append("compiling the reference (%s) failed:\n%s" % (variant, err[-6000:]))
        else:
            os.replace(tmp, so)
    if errors:
        raise RuntimeError("\n".join(errors))
    dt = time.time() - t0 if did else 0.0
    if did or not os.path.isfile(os.path.join(OUT, "BUILD_INFO.txt")):
        ver = subprocess.run(["g++", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
        with open(os.path.join(OUT, "BUILD_INFO.txt"), "w") as f:
            f.write("compiler: %s\n" % ver)
            for variant, flags in VARIANTS.items():
                f.write("%s: g++ -std=c++11 -shared -fPIC %s ... -lpthread\n" % (os.path.basename(lib_path(variant)), " ".join(flags)))
            f.write("sources (unmodified, from the reference tree): %s\n" % " ".join(SOURCES))
            f.write("stand-ins: oracle/ref/opencv2/core/core.hpp, oracle/ref/KeyFrame.h, oracle/ref/Frame.h; C ABI: oracle/ref/harness.cpp\n")
            f.write("build time: %.1f s\n" % dt)
    return dt


if __name__ == "__main__":
    print("reference libraries in %s (%.1f s)" % (OUT, build(force="--force" in sys.argv)))
