#!/bin/bash
# AddressSanitizer + UBSan run of the multigrid-across-ranks host code (rdc_solve.h: rank-local aggregates, coarse ghost layers, send
# and slot lists, device layout with ghost tails) as a stand-alone host program: no device, no Python.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Wno-unknown-pragmas \
  -o tests/_build/host_solve_mg_dist_asan tests/host_solve_mg_dist_main.cpp
tests/_build/host_solve_mg_dist_asan
