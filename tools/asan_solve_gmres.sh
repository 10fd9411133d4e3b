#!/bin/bash
# AddressSanitizer + UBSan run of the GMRES functions of rdc_solve.h (gmres_carve, gmres_givens_step, gmres_back_substitute) as a
# stand-alone host program on buffers of exactly the carved sizes: no device, no Python.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Wno-unknown-pragmas \
  -o tests/_build/host_solve_gmres_asan tests/host_solve_gmres_main.cpp
tests/_build/host_solve_gmres_asan
