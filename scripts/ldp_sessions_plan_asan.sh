#!/bin/sh
# The host-only entries of ethcnn_ldp_sessions_* (ethcnn_ldp_sessions_plan, ethcnn_ldp_sessions_bytes) under AddressSanitizer and
# UndefinedBehaviorSanitizer, as a stand-alone CPU program: tools/ldp_sessions_plan_check.cpp + csrc/ethcnn_ldp_sessions_plan.cpp.
# No GPU, no HIP, nothing loaded into python.  usage: scripts/ldp_sessions_plan_asan.sh [OUTPUT_DIRECTORY]
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
out=${1:-$(mktemp -d)}
mkdir -p "$out"
${CXX:-g++} -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I"$root/include" "$root/tools/ldp_sessions_plan_check.cpp" "$root/hevc-complexity-reduction_amd/csrc/ethcnn_ldp_sessions_plan.cpp" \
    -o "$out/ldp_sessions_plan_check"
exec "$out/ldp_sessions_plan_check"
