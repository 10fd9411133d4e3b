#!/bin/bash
# AddressSanitizer + UBSan run of the two option tables (rdc_options.h) and the validity rule of the solve artefacts
# (rdc_solve_state.h) as a stand-alone host program: no device, no Python.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
  -o tests/_build/host_options_asan tests/host_options_main.cpp
tests/_build/host_options_asan
