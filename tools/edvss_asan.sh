#!/bin/bash
# Build tools/edvss_asan.cpp against the host-only part of the Feldman VSS over Ed25519 (scalars mod L, the
# Lagrange interpolation) and bignum with AddressSanitizer and UndefinedBehaviorSanitizer (host code only, a
# stand-alone program with the GPU entries stubbed) and run it. CPU only.
set -e
cd "$(dirname "$0")/.."
out=${TMPDIR:-/tmp}/mpcx_edvss_asan
H=mpcium_amd/csrc/host
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I $H -I include tools/edvss_asan.cpp \
    $H/edvss.cpp $H/ed25519.cpp $H/bignum.cpp $H/tsscommon.cpp $H/hostprof.cpp -lcrypto -lpthread -o $out
$out
