#!/bin/bash
# tools/build_variant.sh NAME "-DDAL3_ENC_T=2 ..." [SRCDIR]  -> variants/NAME.so (for tools/ab_kernels.py)
# Runs csrc/Makefile with the flags as EXTRA, objects in variants/obj_NAME. SRCDIR: another tree's csrc directory
# (a parent commit's, e.g. from `git archive`), default this tree's.
set -e
cd "$(dirname "$0")/.."
ROOT=$PWD
mkdir -p variants/obj_$1
make -C "${3:-3dal_pytorch_amd/csrc}" -j16 O="$ROOT/variants/obj_$1" OUT="$ROOT/variants/$1.so" EXTRA="$2"
rm -rf variants/obj_$1
echo built variants/$1.so
