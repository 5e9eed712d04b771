#!/bin/bash
# Diagnostic build with s_memtime stamps in fwd_c32_kernel / bwd_c32(_bf16)_kernel (and the unit prologue of the VISIT forms)
# -> tools/ubench/libscone_hip_stamps.so.  Every translation unit, so that the library exports all entry points.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"; ROOT="$(cd "$HERE/.." && pwd)"; C="$ROOT/scone_gcn_amd/csrc"
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -I$ROOT/include -I$C -DSCN_STAMPS ${SCN_EXTRA_FLAGS:-}"
TMP="$(mktemp -d)"
trap 'rm -rf "$TMP"' EXIT
pids=()
for src in "$C"/*.hip; do /opt/rocm/bin/hipcc $FLAGS -c "$src" -o "$TMP/$(basename "$src" .hip).o" & pids+=($!); done
for p in "${pids[@]}"; do wait "$p"; done
mkdir -p "$HERE/ubench"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$HERE/ubench/libscone_hip_stamps.so" "$TMP"/*.o
echo built
