#!/bin/bash
# Builds build/variants/lib_<name>.so: the library with extra device-code defines (A/B experiments; tooling).
#   scripts/build_variant.sh <name> "<extra hipcc flags>"      e.g.  scripts/build_variant.sh wpe4 "-DPPT_TRACE_WPE(s)=4"
#   HOST_DEFS="-DPPT_SAH_BINS=32" scripts/build_variant.sh bins32 ""     also compiles the host code with these defines
# Sources and flags are the Makefile's (make variant); the objects go to build/variants/<name>/.
set -e
cd "$(dirname "$0")/../prosper_amd/csrc"
name=$1; shift
[ -n "$name" ] || { echo "usage: $0 <name> \"<extra hipcc flags>\"" >&2; exit 2; }
rm -rf "../../build/variants/$name"
VARIANT_DEVFLAGS="$*" VARIANT_HOSTFLAGS="$HOST_DEFS" make -s -j16 variant VARIANT="$name"
echo built build/variants/lib_$name.so
