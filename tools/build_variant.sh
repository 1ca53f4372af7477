#!/bin/bash
# Build an A/B variant of the library: tools/build_variant.sh NAME [extra hipcc flags for every source]
# -> build/variants/libnbody_NAME.so   (compare with tools/ab_force.py --libs a=...,b=...)
# The sources and their per-source flags are those of n_body_problem_amd/build.py (SOURCES, EXTRA_FLAGS).
set -e
name=$1; shift
cd "$(dirname "$0")/.."
mkdir -p build/variants/obj_$name
python3 -c 'from n_body_problem_amd import build
for s in build.SOURCES: print(s[:-4], *build.EXTRA_FLAGS.get(s, []))' | while read -r f extra; do
  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off $extra "$@" -c n_body_problem_amd/csrc/$f.hip -o build/variants/obj_$name/$f.o
done
hipcc -shared -fPIC --offload-arch=gfx950 build/variants/obj_$name/*.o -L/opt/rocm/lib -lrccl -o build/variants/libnbody_$name.so
echo build/variants/libnbody_$name.so
