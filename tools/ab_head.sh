#!/bin/bash
# tools/ab_head.sh [rev]  -> build/ab/liblcr_head.so = liblcr built from the sources of <rev> (default HEAD), for a same-box A/B of the
# working tree against it: on the GPU box, alternate `LCR_LIB=build/ab/liblcr_head.so python bench.py --quick ...` and the default library.
# Builds whatever *.hip / *.cpp that revision's csrc holds (no list of its own: tools/build_variant.sh does the compiling).
set -e
cd "$(dirname "$0")/.."
rev=${1:-HEAD}
rm -rf build/ab/old_src; mkdir -p build/ab/old_src
git archive $rev longcallr_amd/csrc include | tar -x -C build/ab/old_src
LCR_SRC=build/ab/old_src/longcallr_amd/csrc tools/build_variant.sh head -Wno-unused-value -w
rm -rf build/ab/old_src
ls -la build/ab/liblcr_head.so
