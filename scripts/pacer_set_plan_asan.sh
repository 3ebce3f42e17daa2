#!/bin/sh
# The host-only entry of ethcnn_pacer_set_* (ethcnn_pacer_set_plan) under AddressSanitizer and UndefinedBehaviorSanitizer, as a
# stand-alone CPU program: tools/pacer_set_plan_check.cpp + csrc/ethcnn_pacer_set_plan.cpp.
# No GPU, no HIP, nothing loaded into python.  usage: scripts/pacer_set_plan_asan.sh [OUTPUT_DIRECTORY]
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
out=${1:-$(mktemp -d)}
mkdir -p "$out"
${CXX:-g++} -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I"$root/include" "$root/tools/pacer_set_plan_check.cpp" "$root/hevc-complexity-reduction_amd/csrc/ethcnn_pacer_set_plan.cpp" \
    -o "$out/pacer_set_plan_check"
exec "$out/pacer_set_plan_check"
