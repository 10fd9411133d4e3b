#!/bin/bash
# AddressSanitizer + UBSan run of the colouring of the Gauss-Seidel smoother (rdc_solve.h: mg_colour, mg_gs_place) as a
# stand-alone host program: no device, no Python.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Wno-unknown-pragmas \
  -o tests/_build/host_solve_mg_gs_asan tests/host_solve_mg_gs_main.cpp
tests/_build/host_solve_mg_gs_asan
