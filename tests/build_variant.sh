#!/bin/bash
# Experiment builds of the product library with compile-time knobs, for A/B timing on the box:
#   tests/build_variant.sh <name> -DKNOB=VALUE ...  ->  build_exp/<name>/libsiftgpu.so
# Load one with SGPU_LIB_PATH=build_exp/<name>/libsiftgpu.so (tests/probe.py, bench.py).
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/build_exp/$NAME
mkdir -p "$OUT"
PKG=$ROOT/modify-sift-gpu_amd
# one source list: the product Makefile, with its outputs redirected and the knobs appended
make -C "$PKG" -j8 BUILD="$OUT/obj" LIB="$OUT" EXTRA_DEFS="$*" "$OUT/libsiftgpu.so"
rm -rf "$OUT/obj"
# the test-hook library is loaded from beside the product library (sgpu_debug_candidates)
cp "$PKG/lib/libsiftgpu_debug.so" "$OUT/"
# a kernel whose host stub was not emitted links into the .so and fails only when loaded
if nm -D --undefined-only "$OUT/libsiftgpu.so" | grep -q __device_stub; then echo "undefined kernel stubs in $OUT"; exit 1; fi
echo "built $OUT/libsiftgpu.so"
