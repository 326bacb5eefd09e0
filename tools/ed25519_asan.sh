#!/bin/bash
# Build tools/ed25519_asan.cpp against the host Ed25519 arithmetic and bignum with AddressSanitizer and
# UndefinedBehaviorSanitizer (host code only, a stand-alone program) and run it. CPU only.
set -e
cd "$(dirname "$0")/.."
out=${TMPDIR:-/tmp}/mpcx_ed25519_asan
H=mpcium_amd/csrc/host
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I $H tools/ed25519_asan.cpp \
    $H/ed25519.cpp $H/bignum.cpp $H/hostprof.cpp -lcrypto -lpthread -o $out
$out
