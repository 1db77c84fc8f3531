#!/bin/bash
# Build and run scripts/vis_host_check.cpp: the index arithmetic of csrc/vis.hip on the CPU under AddressSanitizer and UBSan.
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
src=$here/../masked-diffusion-model_amd/csrc/vis.hip
out=${1:-$(mktemp -d)}
mkdir -p "$out"
awk '/^struct Range/{p=1} /^\/\/ the workgroup.s pair/{p=0} p' "$src" > "$out/range_part.inc"
awk '/^struct GridGeom/{p=1} /^}  \/\/ namespace mdm/{p=0} p' "$src" > "$out/grid_part.inc"
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I"$out" "$here/vis_host_check.cpp" -o "$out/vis_host_check"
"$out/vis_host_check"
