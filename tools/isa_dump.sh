#!/bin/bash
# Dump the gfx950 ISA of one kernel source (for reading waits, spills, loads).
#   tools/isa_dump.sh <outdir> [<file>.hip] [extra hipcc flags...]
# <file>.hip is a name under distributed-grep_amd/csrc/kernels/ or a path;
# default scan_dfa.hip. Writes <outdir>/<file>-hip-amdgcn-amd-amdhsa-gfx950.s
# and prints per kernel: for scan_dfa.hip the scan kernels' VGPRs / LDS /
# scratch, for any other file every kernel's VGPRs / SGPRs / LDS / scratch.
set -euo pipefail
OUT=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
SRC=scan_dfa.hip
if [[ ${1:-} == *.hip ]]; then SRC=$1; shift; fi
# a bare name is the project's kernel source; anything else is a path
if [[ $SRC != */* && -f "$R/distributed-grep_amd/csrc/kernels/$SRC" ]]; then
  SRC="$R/distributed-grep_amd/csrc/kernels/$SRC"
else
  SRC=$(realpath "$SRC")
fi
B=$(basename "$SRC" .hip)
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
cd "$OUT"
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 "$@" -c "$SRC" --save-temps -o "$OUT/$B.o"
S="$OUT/$B-hip-amdgcn-amd-amdhsa-gfx950.s"
meta() { grep -E "^\s+\.($1):" "$S"; }
if [[ $B == scan_dfa ]]; then
  meta "name|vgpr_count|group_segment_fixed_size|private_segment_fixed_size" | paste - - - - |
    grep scan_dfa8 | awk '{print "lds=" $2, "scratch=" $6, "vgpr=" $8, $4}'
else
  meta "name|vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size" | paste - - - - - |
    awk '{print "vgpr=" $10, "sgpr=" $8, "lds=" $2, "scratch=" $6, $4}'
fi
