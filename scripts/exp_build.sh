#!/bin/bash
# Build an experimental variant of libamc_lba.so (every lba_*.hip of the tree) with extra defines into
# amc-slam_amd/lib/exp/<name>.so (load it with AMC_LBA_LIB=<path>): e.g. scripts/exp_build.sh nostore -DLBA_EXP_NOSTORE
set -eu
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
mkdir -p "$ROOT/amc-slam_amd/lib/exp"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared "$@" "$ROOT"/amc-slam_amd/csrc/lba_*.hip \
    -o "$ROOT/amc-slam_amd/lib/exp/$NAME.so" -lrccl
