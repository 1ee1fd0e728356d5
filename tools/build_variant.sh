#!/bin/bash
# builds a measurement variant of libkartohip.so: tools/build_variant.sh <out.so> [--instrumented] <extra hipcc flags...>
# --instrumented: the round-4 measurement scaffolding of the LDS-staged scoring kernels (-DKH_LDS_EXP=n, -DKH_LDS_TIMING, eight waves
# per angle), which left the shipped sources in round 5, is patched back into a scratch copy first
# (tools/patches/r4_k_score_lds_instrumentation.patch; it applies to the matcher_kernels.hip of the commit that added it).
out=$1; shift
src="$(cd "$(dirname "$0")/../slam_toolbox_amd/csrc" && pwd)"
# the library's sources are the ones slam_toolbox_amd/build.py compiles (SOURCES), so that a variant exports the whole ABI
sources=$(cd "$src/.." && python3 -c "import build; print(' '.join(build.SOURCES))") || exit 1
if [ "$1" = "--instrumented" ]; then
  shift
  tmp=$(mktemp -d) && cp "$src"/* "$tmp"/ && (cd "$tmp" && patch -p3 < "$src/../../tools/patches/r4_k_score_lds_instrumentation.patch") || exit 1
  src=$tmp
fi
cd "$src"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -fvisibility=hidden -Wno-unused-value -shared -ldl "$@" -o "$out" \
  $sources
