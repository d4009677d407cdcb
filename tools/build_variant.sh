#!/bin/bash
# build a kernel variant of liborbx.so into tools/bin/: tools/build_variant.sh NAME -DFR_WPS=5 ...
# (the source list and the base flags are build.py's: a variant differs from the package's library by the flags given here alone)
name=$1; shift
cd "$(dirname "$0")/.."
exec python3 -c 'import sys; sys.path.insert(0, "orb_slam2_detailed_comments_amd"); import build
build.build(out=sys.argv[1], extra=["-w"] + sys.argv[2:])' tools/bin/liborbx_$name.so "$@"
