#!/bin/bash
# AddressSanitizer + UBSan run of the host code of rdc_solid_newton_dist (rdc_newton.h: newton_linear_dispatch, newton_comm_complete,
# newton_carve_dist) as a stand-alone host program: no device, no Python.  Every (precond, method), a few callback sets, the layouts
# of the cube on three ranks, of a rank that owns nothing and of 2^30 nodes.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Wno-unknown-pragmas \
  -o tests/_build/host_newton_dist_asan tests/host_newton_dist_main.cpp
{
  for p in -1 0 1 2 3 4 5 6 7; do for m in 0 1 2; do echo "dispatch $p $m"; done; done
  for p in 2 3 5 6; do for m in 0 1; do for mask in 0 7 31 39 63; do echo "complete $p $m $mask"; done; done; done
  echo "carve 729 729"
  echo "carve_dist 729 729 0"
  echo "carve_dist 391 300 95"
  echo "carve_dist 355 239 140"
  echo "carve_dist 289 190 104"
  echo "carve_dist 40 0 0"
  echo "carve_dist 0 0 0"
  echo "carve_dist 1073741824 1073741819 1048576"
} | tests/_build/host_newton_dist_asan
