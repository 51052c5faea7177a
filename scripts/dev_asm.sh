#!/bin/bash
# Device assembly of one unit of csrc/ (default decoder.hip) with the library's flags (for
# scripts/isa_stats.py):
#   bash scripts/dev_asm.sh out.s [UNIT.hip] [EXTRA_FLAGS...]
set -eu
R="$(cd "$(dirname "$0")/.." && pwd)"
C="$R/qam-reconciliation_amd/csrc"
out=$1; shift
unit=decoder.hip
if [ $# -gt 0 ] && [ "${1%.hip}" != "$1" ]; then unit=$1; shift; fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math \
    -I"$R/include" -I"$C/build" --cuda-device-only -S "$@" -o "$out" "$C/$unit"
