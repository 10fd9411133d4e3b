#!/bin/bash
# AddressSanitizer + UBSan run of the host+device functions of the block ILU(0) on patterns with ghost columns (rdc_solve.h:
# ilu_build with ghosts, ilu_value_offset, ilu_find, ilu_factor_node over the owned positions, ilu_place with a ghost tail) as a
# stand-alone host program: no device, no Python.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Wno-unknown-pragmas \
  -o tests/_build/host_solve_ilu_dist_asan tests/host_solve_ilu_dist_main.cpp
tests/_build/host_solve_ilu_dist_asan
