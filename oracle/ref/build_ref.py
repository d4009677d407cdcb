"""Compiles the reference's own sources, unmodified and straight from the reference tree, into oracle/_ref/ (kept out of git):
DBoW2 and KeyFrameDatabase behind the stand-in headers of this directory and the C ABI of harness.cpp, and ORBmatcher and
MapPoint behind the stand-ins of matcher/ and the C ABI of matcher/harness.cpp (that of tests/compat_runtime/harness.cpp):

    libref_dbow2_strict.so   g++ -O3 -ffp-contract=off    what fp_mode = FP_STRICT stands for
    libref_dbow2_fma.so      g++ -O3 -mfma                what fp_mode = FP_GCC_FMA stands for (GCC contracts a * b + c where its
                                                          default -ffp-contract=fast allows it; an explicit ISA flag, not
                                                          -march=native, because the binaries travel to other machines)
    libref_matcher_strict.so, libref_matcher_fma.so     the same two flag sets for src/ORBmatcher.cc and src/MapPoint.cc; the
                                                          feature grid behind GetFeaturesInArea is the oracle's (orb_oracle_match.c,
                                                          compiled with the oracle's own flags and linked in)
    libref_extractor_strict.so, libref_extractor_fma.so the same two flag sets for src/ORBextractor.cc behind the stand-ins of
                                                          extractor/ and the C ABI of extractor/harness.cpp; the six OpenCV primitives
                                                          forward to the oracle's (orb_oracle.c, compiled with the oracle's own flags
                                                          and linked in); std::list nodes come from a monotonic arena (F3)
    libref_extractor_strict_plain.so                    the strict flags with glibc malloc instead of the arena: one measurement
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
MATCHER = os.path.join(HERE, "matcher")
MATCHER_SOURCES = ["src/ORBmatcher.cc", "src/MapPoint.cc", "Thirdparty/DBoW2/DBoW2/FeatureVector.cpp", "Thirdparty/DBoW2/DBoW2/BowVector.cpp"]
MATCHER_STANDINS = ["Map.h", "KeyFrame.h", "Frame.h", "grid.h", "opencv2/core/core.hpp", "opencv2/features2d/features2d.hpp", "opencv/cv.h"]
EXTRACTOR = os.path.join(HERE, "extractor")
EXTRACTOR_SOURCES = ["src/ORBextractor.cc", "include/ORBextractor.h"]   # the first is #included by extractor/harness.cpp
EXTRACTOR_STANDINS = ["opencv2/core/core.hpp", "opencv2/features2d/features2d.hpp", "opencv2/highgui/highgui.hpp",
                      "opencv2/imgproc/imgproc.hpp", "opencv/cv.h"]
EXTRACTOR_BUILDS = {"strict": ("strict", []), "fma": ("fma", []), "strict_plain": ("strict", ["-DREF_PLAIN_MALLOC"])}
ORACLE_C = ["orb_oracle_match.c", "orb_oracle.c"]                      # the grid, and what it links against
ORACLE_CFLAGS = ["-O2", "-fPIC", "-std=gnu99", "-ffp-contract=off", "-fno-fast-math", "-w"]   # oracle/Makefile's
VARIANTS = {"strict": ["-O3", "-ffp-contract=off"], "fma": ["-O3", "-mfma"]}


def reference_dir():
    return os.environ.get("ORB_SLAM2_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))


def reference_present():
    ref = reference_dir()
    return all(os.path.isfile(os.path.join(ref, s)) for s in SOURCES + MATCHER_SOURCES + EXTRACTOR_SOURCES)


def lib_path(variant):
    return os.path.join(OUT, "libref_dbow2_%s.so" % variant)


def matcher_lib_path(variant):
    return os.path.join(OUT, "libref_matcher_%s.so" % variant)


def extractor_lib_path(build):
    return os.path.join(OUT, "libref_extractor_%s.so" % build)


def extractor_built():
    return all(os.path.isfile(extractor_lib_path(b)) for b in EXTRACTOR_BUILDS)


def built():
    return all(os.path.isfile(lib_path(v)) for v in VARIANTS)


def matcher_built():
    return all(os.path.isfile(matcher_lib_path(v)) for v in VARIANTS)


def command(variant, out):
    ref = reference_dir()
    # -include: the stand-ins define the include guards of the reference's KeyFrame.h / Frame.h before KeyFrameDatabase.h
    # includes its siblings by quoted name; -I HERE first: <opencv2/core/core.hpp> is the stand-in
    return (["g++", "-std=c++11", "-w", "-shared", "-fPIC"] + VARIANTS[variant] +
            ["-I" + HERE, "-I" + ref, "-I" + os.path.join(ref, "include"),
             "-include", os.path.join(HERE, "KeyFrame.h"), "-include", os.path.join(HERE, "Frame.h")] +
            [os.path.join(ref, s) for s in SOURCES] + [os.path.join(HERE, "harness.cpp"), "-lpthread", "-o", out])


def matcher_command(variant, out, extra=()):
    """one shell line: the oracle's two C files to objects under the oracle's flags (the grid must not change with the variant),
    then the reference sources and the harness with the variant's flags, linked together; the objects are removed again"""
    ref = reference_dir()
    oracle = os.path.dirname(HERE)
    objs = ["%s.%s.o" % (out, os.path.splitext(c)[0]) for c in ORACLE_C]
    cc = [["gcc"] + ORACLE_CFLAGS + ["-c", os.path.join(oracle, c), "-o", o] for c, o in zip(ORACLE_C, objs)]
    # the three stand-ins define the include guards of the reference's Map.h / KeyFrame.h / Frame.h, which MapPoint.h and
    # ORBmatcher.h include by quoted name (their own siblings first); -I MATCHER first: <opencv2/...> and <opencv/cv.h> are stand-ins
    link = (["g++", "-std=c++11", "-w", "-shared", "-fPIC"] + VARIANTS[variant] + list(extra) +
            ["-I" + MATCHER, "-I" + oracle, "-I" + ref, "-I" + os.path.join(ref, "include"),
             "-include", os.path.join(MATCHER, "Map.h"), "-include", os.path.join(MATCHER, "KeyFrame.h"),
             "-include", os.path.join(MATCHER, "Frame.h")] +
            [os.path.join(ref, s) for s in MATCHER_SOURCES] + [os.path.join(MATCHER, "harness.cpp")] + objs +
            ["-lpthread", "-lm", "-o", out])
    q = lambda c: " ".join("'%s'" % a for a in c)
    return ["sh", "-c", " && ".join(q(c) for c in cc + [link]) + "; rc=$?; rm -f " + q(objs) + "; exit $rc"]


def extractor_command(build, out, extra=()):
    """as matcher_command: the oracle's C files under the oracle's flags (the primitives must not change with the variant), then
    extractor/harness.cpp, which #includes <src/ORBextractor.cc> from the reference, with the variant's flags"""
    ref = reference_dir()
    oracle = os.path.dirname(HERE)
    variant, defs = EXTRACTOR_BUILDS[build]
    objs = ["%s.%s.o" % (out, os.path.splitext(c)[0]) for c in ORACLE_C]
    cc = [["gcc"] + ORACLE_CFLAGS + ["-c", os.path.join(oracle, c), "-o", o] for c, o in zip(ORACLE_C, objs)]
    link = (["g++", "-std=c++11", "-w", "-shared", "-fPIC"] + VARIANTS[variant] + defs + list(extra) +
            ["-I" + EXTRACTOR, "-I" + oracle, "-I" + ref, "-I" + os.path.join(ref, "include"),
             os.path.join(EXTRACTOR, "harness.cpp")] + objs +
            ["-Wl,--version-script=" + os.path.join(EXTRACTOR, "exports.map"), "-lm", "-o", out])
    q = lambda c: " ".join("'%s'" % a for a in c)
    return ["sh", "-c", " && ".join(q(c) for c in cc + [link]) + "; rc=$?; rm -f " + q(objs) + "; exit $rc"]


def build(force=False):
    """Returns the seconds spent compiling (0.0 when everything is up to date)."""
    if not reference_present():
        raise FileNotFoundError("reference tree not found at %s (set ORB_SLAM2_REFERENCE)" % reference_dir())
    if shutil.which("g++") is None:
        raise RuntimeError("g++ not found")
    os.makedirs(OUT, exist_ok=True)
    mine = [os.path.join(HERE, f) for f in ("harness.cpp", "KeyFrame.h", "Frame.h", "build_ref.py", "opencv2/core/core.hpp")]
    deps = mine + [os.path.join(reference_dir(), s) for s in SOURCES]
    oracle = os.path.dirname(HERE)
    mdeps = ([os.path.join(MATCHER, f) for f in MATCHER_STANDINS + ["harness.cpp"]] + [os.path.join(HERE, "build_ref.py")] +
             [os.path.join(ROOT, "tests", "compat_runtime", "opencv2", "core", "core.hpp")] +
             [os.path.join(oracle, f) for f in ORACLE_C + ["orb_oracle.h", os.path.join("..", "include", "orbx_rect_digest.h")]] + [os.path.join(reference_dir(), s) for s in MATCHER_SOURCES])
    xdeps = ([os.path.join(EXTRACTOR, f) for f in EXTRACTOR_STANDINS + ["harness.cpp", "exports.map"]] + [os.path.join(HERE, "build_ref.py")] +
             [os.path.join(oracle, f) for f in ORACLE_C + ["orb_oracle.h", os.path.join("..", "include", "orbx_rect_digest.h")]] + [os.path.join(reference_dir(), s) for s in EXTRACTOR_SOURCES])
    t0 = time.time()
    jobs = []
    for path, cmd, dd, names in ((lib_path, command, deps, VARIANTS), (matcher_lib_path, matcher_command, mdeps, VARIANTS),
                                 (extractor_lib_path, extractor_command, xdeps, EXTRACTOR_BUILDS)):
        newest = max(os.path.getmtime(d) for d in dd)
        for variant in names:               # all builds side by side
            so = path(variant)
            if not force and os.path.isfile(so) and os.path.getmtime(so) >= newest:
                continue
            tmp = so + ".tmp%d" % os.getpid()
            jobs.append((os.path.basename(so), so, tmp, subprocess.Popen(cmd(variant, tmp), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)))
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
            for variant, flags in VARIANTS.items():
                f.write("%s: g++ -std=c++11 -shared -fPIC %s ... -lpthread -lm\n" % (os.path.basename(matcher_lib_path(variant)), " ".join(flags)))
            f.write("matcher sources (unmodified, from the reference tree): %s\n" % " ".join(MATCHER_SOURCES))
            f.write("matcher stand-ins: %s, tests/compat_runtime/opencv2/core/core.hpp (cv::Mat); C ABI: oracle/ref/matcher/harness.cpp\n"
                    % ", ".join("oracle/ref/matcher/" + m for m in MATCHER_STANDINS))
            f.write("matcher feature grid (ours, restated): %s, gcc %s\n" % (" ".join("oracle/" + c for c in ORACLE_C), " ".join(ORACLE_CFLAGS)))
            for b, (variant, defs) in EXTRACTOR_BUILDS.items():
                f.write("%s: g++ -std=c++11 -shared -fPIC %s ... -lm\n" % (os.path.basename(extractor_lib_path(b)), " ".join(VARIANTS[variant] + defs)))
            f.write("extractor sources (unmodified, from the reference tree, #included by the harness): %s\n" % " ".join(EXTRACTOR_SOURCES))
            f.write("extractor stand-ins: %s; C ABI: oracle/ref/extractor/harness.cpp\n" % ", ".join("oracle/ref/extractor/" + m for m in EXTRACTOR_STANDINS))
            f.write("extractor OpenCV primitives (ours, restated): %s, gcc %s\n" % (" ".join("oracle/" + c for c in ORACLE_C), " ".join(ORACLE_CFLAGS)))
            f.write("build time: %.1f s\n" % dt)
    return dt


if __name__ == "__main__":
    print("reference libraries in %s (%.1f s)" % (OUT, build(force="--force" in sys.argv)))
