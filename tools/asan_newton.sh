#!/bin/bash
# AddressSanitizer + UBSan run of the Newton host code (rdc_newton.h: newton_next, newton_carve, newton_check_params) as a
# stand-alone host program: no device, no Python.  The script drives a run with halvings, a stop by step and a NaN residual.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Wno-unknown-pragmas \
  -o tests/_build/host_newton_asan tests/host_newton_main.cpp
tests/_build/host_newton_asan <<'SCRIPT'
constants
sizes
carve 729 729
carve 1073741824 1073741824
check 10 0 1e-3 1e-8 1e-8 1e-3 0 50000 2 0
check 0 0 nan 1e-8 1e-8 1e-3 0 50000 9 0
run 10 1 0 1e-8 1e-8 8
100 0 0 0 0
0 0 0 0 7
500 1 10 0 0
100 0.5 10 0 0
99 0.25 10 0 0
0 0 0 0 0
nan 0 0 0 0
0 0 0 0 0
run 10 0 1e-3 1e-8 1e-8 4
1000 0 0 0 0
0 0 0 1 9
0 1e-3 1 0 0
0.25 0 0 0 0
SCRIPT
