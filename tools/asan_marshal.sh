#!/bin/bash
# AddressSanitizer + UBSan run of the host marshalling header (include/rdc_marshal.h) as a stand-alone host program: every key
# table read through both parameter stores, the solid pieces, and the pipelined hand-back against the fake of its five C-ABI
# calls over (n_nodes, n_chunks) = (27, 1), (27, 2), (27, 7), (5, 40).  No device, no library, no Python.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
  -o tests/_build/host_marshal_asan tests/host_marshal_main.cpp tests/fake_rdc_handback.cpp
tests/_build/host_marshal_asan > /dev/null
tests/_build/host_marshal_asan tables > /dev/null
echo "host_marshal_asan: clean"
