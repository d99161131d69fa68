#!/bin/bash
# tools/build_variant.sh NAME "EXTRA FLAGS"  -> build/ab/liblcr_NAME.so (A/B timing of kernel variants: LCR_LIB=... on the GPU box)
# Compiles every *.hip (device flags) and *.cpp (host only) of longcallr_amd/csrc, or of the directory LCR_SRC names (tools/ab_head.sh).
set -e
cd "$(dirname "$0")/.."
name=$1; shift
src=${LCR_SRC:-longcallr_amd/csrc}
out=build/ab
obj=$out/obj_$name
rm -rf $obj; mkdir -p $obj
pids=""
for f in $src/*.hip; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function "$@" -c $f -o $obj/$(basename $f .hip).o & pids="$pids $!"
done
for f in $src/*.cpp; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC "$@" -c $f -o $obj/$(basename $f .cpp).o & pids="$pids $!"
done
for p in $pids; do wait $p; done   # (set -e: a failed compile ends the script here, not at a link with objects missing)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o $out/liblcr_$name.so $obj/*.o -lz
rm -rf $obj
echo $out/liblcr_$name.so
