#!/bin/bash
# AddressSanitizer + UBSan run of what the rank-local Gauss-Seidel smoother across ranks (precond 6) adds on the host (rdc_solve.h:
# mg_colour on the levels of ghosted hierarchies, a rank that owns nothing included, mg_gs_interior, mg_gs_place) as a stand-alone
# host program: no device, no Python.  (The program takes in the text of host_solve_mg_dist_main.cpp, whose own checks it does not call.)
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Wno-unknown-pragmas \
  -Wno-unused-function -o tests/_build/host_solve_mg_gs_dist_asan tests/host_solve_mg_gs_dist_main.cpp
tests/_build/host_solve_mg_gs_dist_asan
