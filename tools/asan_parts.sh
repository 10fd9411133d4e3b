#!/bin/bash
# AddressSanitizer + UBSan run of the two-part splits (rdc_parts.h) on the lists of a K(6) mesh, as a stand-alone host
# program: no device, no Python.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
  -o tests/_build/host_parts_asan tests/host_parts_main.cpp rdcfes_amd/csrc/rdc_meshprep.cpp rdcfes_amd/csrc/rdc_prep_ev.cpp
tests/_build/host_parts_asan
