// pacer_set_plan_check.cpp -- a stand-alone host program over the host-only entry of ethcnn_pacer_set_* (include/ethcnn.h):
// ethcnn_pacer_set_plan with the inputs of tests/test_pacer_set_cpu.py, each result held against the definition, output arrays of exactly
// the documented sizes.  Meant for a sanitizer build on the CPU (scripts/pacer_set_plan_asan.sh: -fsanitize=address,undefined over this
// file and csrc/ethcnn_pacer_set_plan.cpp); no GPU, no HIP.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ethcnn.h"

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

static void check_plan(const std::vector<int64_t>& nctus, int64_t K) {
    const size_t n = nctus.size();
    // exactly n entries each: a write behind them is the sanitizer's to find
    std::vector<int64_t> cf(n, -1), cb(n, -1), bf(n, -1), r0(n, -1);
    std::vector<int32_t> sl(n, -1);
    int64_t cg = -1, bg = -1;
    EXPECT(ethcnn_pacer_set_plan(nctus.data(), (int)n, K, cf.data(), cb.data(), sl.data(), bf.data(), r0.data(), &cg, &bg) == ETHCNN_OK);
    const int64_t rung_blocks = (K + 1 + 255) / 256;
    int64_t count = 0, bake = 0, rec = 0;
    for (size_t j = 0; j < n; ++j) {
        const int64_t per = nctus[j], most = (per + 63) / 64, len = (per + most - 1) / most, slices = (per + len - 1) / len;
        EXPECT(sl[j] == len && len >= 1 && len <= 64 && (slices - 1) * len < per && slices * len >= per);
        EXPECT(cf[j] == count && cb[j] == slices * rung_blocks);
        EXPECT(bf[j] == bake && r0[j] == rec);
        count += cb[j], bake += (per + 255) / 256, rec += per;
    }
    EXPECT(cg == count && bg == bake);
    // any output may be left out
    int64_t only = -1;
    EXPECT(ethcnn_pacer_set_plan(nctus.data(), (int)n, K, nullptr, nullptr, nullptr, nullptr, nullptr, &only, nullptr) == ETHCNN_OK && only == count);
    EXPECT(ethcnn_pacer_set_plan(nctus.data(), (int)n, K, nullptr, nullptr, nullptr, nullptr, r0.data(), nullptr, nullptr) == ETHCNN_OK);
}

int main() {
    std::vector<std::vector<int64_t>> calls = {{1}, {12}, {64}, {65}, {272}, {1, 12, 272}, {272, 1, 12}, {64, 65, 1}};
    std::vector<int64_t> mixed;
    for (int j = 0; j < 32; ++j) mixed.push_back(1 + (j * 37) % 300);
    calls.push_back(mixed);
    calls.push_back(std::vector<int64_t>(32, (1 << 24) - 1));  // the largest call there is: 2^29 records, 2^35 bytes of them
    for (const auto& c : calls)
        for (int64_t K : {1, 255, 256, 513, 4096}) check_plan(c, K);

    const int64_t two[2] = {4, 12}, zero[2] = {4, 0}, big[1] = {1 << 24}, neg[1] = {-1};
    const std::vector<int64_t> many(33, 1);
    int64_t out[33], grid = 7;
    int32_t len[33];
    EXPECT(ethcnn_pacer_set_plan(two, 2, 512, out, out, len, out, out, &grid, &grid) == ETHCNN_OK);
    grid = 7;
    EXPECT(ethcnn_pacer_set_plan(zero, 2, 512, out, out, len, out, out, &grid, &grid) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_pacer_set_plan(big, 1, 512, out, out, len, out, out, &grid, &grid) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_pacer_set_plan(neg, 1, 512, out, out, len, out, out, &grid, &grid) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_pacer_set_plan(two, 0, 512, out, out, len, out, out, &grid, &grid) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_pacer_set_plan(many.data(), 33, 512, out, out, len, out, out, &grid, &grid) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_pacer_set_plan(two, 2, 0, out, out, len, out, out, &grid, &grid) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_pacer_set_plan(two, 2, 4097, out, out, len, out, out, &grid, &grid) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_pacer_set_plan(nullptr, 2, 512, out, out, len, out, out, &grid, &grid) == ETHCNN_ERR_ARG);
    EXPECT(grid == 7);  // a refusal writes nothing
    std::printf("pacer_set_plan_check: %zu calls, %d failures\n", calls.size(), failures);
    return failures ? 1 : 0;
}
