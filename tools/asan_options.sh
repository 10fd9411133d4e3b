#!/bin/bash
# AddressSanitizer + UBSan run of the option table (rdc_options.h) as a stand-alone host program: no device, no Python.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
  -o tests/_build/host_options_asan tests/host_options_main.cpp
tests/_build/host_options_asan
