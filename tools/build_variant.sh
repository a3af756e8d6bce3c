#!/bin/bash
# An experimental build of libsf_hip.so with extra compiler flags, beside the product library (A/B runs: SF_HIP_LIB).
#   tools/build_variant.sh NAME "EXTRA FLAGS" [SOURCE_DIR]   ->   staticfusion_amd/csrc/libsf_hip_NAME.so
# SOURCE_DIR defaults to this tree's staticfusion_amd/csrc (give a checkout of another revision to build that one).
# O5FLAGS in the environment replaces -DSF_OCC=5 of the 5-per-CU frame object. The objects and their flags are the
# product's: this runs the product's rule of this tree's csrc/Makefile on SOURCE_DIR, with the objects in a directory of their own.
set -eu
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; EXTRA=${2:-}; SRC=${3:-$ROOT/staticfusion_amd/csrc}
OUT=$ROOT/staticfusion_amd/csrc; OBJ=${TMPDIR:-/tmp}/sf_variant_$NAME; rm -rf "$OBJ"; mkdir -p "$OBJ"
make -C "$SRC" -f "$OUT/Makefile" -j8 EXTRA_HIPFLAGS="$EXTRA" O5FLAGS="${O5FLAGS:--DSF_OCC=5}" OBJDIR="$OBJ/" \
    PRODUCT="$OUT/libsf_hip_$NAME.so" "$OUT/libsf_hip_$NAME.so"
echo built "$OUT/libsf_hip_$NAME.so"
