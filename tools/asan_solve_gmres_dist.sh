#!/bin/bash
# AddressSanitizer + UBSan run of the partitioned form of the GMRES state of rdc_solve.h (gmres_carve with n_nodes: ghosted basis
# slots, the buffer of the wide all-reduce) as a stand-alone host program on buffers of exactly the carved sizes: no device, no Python.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Wno-unknown-pragmas \
  -o tests/_build/host_solve_gmres_dist_asan tests/host_solve_gmres_dist_main.cpp
tests/_build/host_solve_gmres_dist_asan
