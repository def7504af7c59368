#!/bin/bash
# Build host_trace.cpp against a given libcara_hip.so and write one trace per setting of the switches into a directory.
#   tools/host_trace/trace.sh <path/to/libcara_hip.so> <out_dir>
# Run it on the library before a change and after it, then `diff -r` the two directories: a refactor of vit.hip's host code leaves
# every file byte-identical.  No GPU is needed (nothing is launched).  50 settings below, one .trace file each:
#   * 45 without HOST_TRACE_POOL: the 16 token-readout shapes of host_trace.cpp (SHAPES), each with inference 0 and 1: the workspace
#     size, the four forward entries and the backward.  These files hold token-readout shapes only and are the ones to compare across
#     a change that must leave the token path alone.
#   * 5 with HOST_TRACE_POOL=1: the 7 shapes of the mean-pooled readout (POOLED, cara_vit_shape::pool = 1) in SHAPES' place, the same
#     entries; one of the 7 asks for exact weight dropout, which the pooled readout refuses: workspace size 0 and status 1 from every entry.
set -euo pipefail
LIB=$(realpath "$1")
OUT=$2
HERE=$(cd "$(dirname "$0")" && pwd)
mkdir -p "$OUT"
EXE=$OUT/host_trace
LIBDIR=$(dirname "$LIB")
# (-rdynamic: the executable's definitions must be in its dynamic symbol table to take precedence over the libraries')
${CXX:-g++} -std=c++17 -O1 -rdynamic -o "$EXE" "$HERE/host_trace.cpp" "$LIB" -ldl -Wl,-rpath,"$LIBDIR" -Wl,--allow-shlib-undefined

# the switches, one setting per line ("-" = the defaults)
SETTINGS=$(cat <<'EOF'
-
CARA_EPI_RIDERS=1
CARA_FC1_SIDE=1
CARA_DV=1
CARA_DV=2
CARA_DV=3
CARA_EPI_RIDERS=1 CARA_FC1_SIDE=1
CARA_EPI_RIDERS=1 CARA_DV=3
CARA_FC1_SIDE=1 CARA_DV=2
CARA_FC1_SIDE=1 CARA_DV=3
CARA_GEMM8=0
CARA_EPI_RIDERS=1 CARA_GEMM8=0
CARA_FC1_SIDE=1 CARA_GEMM8=0
CARA_DV=3 CARA_GEMM8=0
CARA_GEMM8_HELPERS=1
CARA_DV=3 CARA_GEMM8_HELPERS=1
CARA_EPI_RIDERS=1 CARA_GEMM8_HELPERS=1
CARA_GEMM8_MAXK_TS=3072
CARA_DV=3 CARA_GEMM8_MAXK_TS=3072
CARA_ER_ROWS=160
CARA_EPI_RIDERS=1 CARA_ER_ROWS=160
CARA_CLS_SHORTCUT=0
CARA_EPI_RIDERS=1 CARA_CLS_SHORTCUT=0
CARA_DV=3 CARA_CLS_SHORTCUT=0
CARA_FC1_SIDE=1 CARA_CLS_SHORTCUT=0
CARA_GEMM_G_INSIDE=0
CARA_GEMM_G_INSIDE=1
CARA_GEMM_G_INSIDE=2
CARA_DV=3 CARA_GEMM_G_INSIDE=1
CARA_FUSE_TS=0
CARA_LN2B_XU=0
CARA_PANEL_ACTS=0
CARA_PANEL_ACTS=7
CARA_FUSE_XU=0
CARA_BWD_MEMSETS=1
CARA_SAVE_GELU_GRAD=0
CARA_SAVE_GELU_GRAD=1
CARA_CLS_ATTN=0
CARA_FUSE_GEMM_T=0
CARA_GEMM_PACKED=0
CARA_EPI_RIDERS=1 CARA_SAVE_GELU_GRAD=0
HOST_TRACE_SITES=1
HOST_TRACE_SITES=1 CARA_EPI_RIDERS=1
HOST_TRACE_SITES=1 CARA_FC1_SIDE=1
HOST_TRACE_SITES=1 CARA_CLS_SHORTCUT=0
HOST_TRACE_POOL=1
HOST_TRACE_POOL=1 CARA_PANEL_ACTS=0
HOST_TRACE_POOL=1 CARA_PANEL_ACTS=7
HOST_TRACE_POOL=1 CARA_EPI_RIDERS=1
HOST_TRACE_POOL=1 HOST_TRACE_SITES=1
EOF
)
while IFS= read -r setting; do
  name=$(echo "$setting" | tr ' =' '_-')
  [ "$setting" = "-" ] && { setting=""; name=default; }
  env -i PATH="$PATH" LD_LIBRARY_PATH="${LD_LIBRARY_PATH:-}" $setting "$EXE" > "$OUT/$name.trace"
done <<< "$SETTINGS"
rm -f "$EXE"
wc -l "$OUT"/*.trace | tail -n 1
