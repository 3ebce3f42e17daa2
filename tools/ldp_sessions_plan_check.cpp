// ldp_sessions_plan_check.cpp -- a stand-alone host program over the two host-only entries of ethcnn_ldp_sessions_* (include/ethcnn.h):
// ethcnn_ldp_sessions_plan and ethcnn_ldp_sessions_bytes with the inputs of tests/test_ldp_sessions_cpu.py, each result held against
// the definition, output arrays of exactly the documented sizes.  Meant for a sanitizer build on the CPU
// (scripts/ldp_sessions_plan_asan.sh: -fsanitize=address,undefined over this file and csrc/ethcnn_ldp_sessions_plan.cpp); no GPU, no HIP.
#include <algorithm>
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

static void check_plan(const std::vector<int>& nctus, int cap) {
    const int n = (int)nctus.size();
    std::vector<int> first(n, -1);
    int npasses = -1;
    EXPECT(ethcnn_ldp_sessions_plan(nctus.data(), n, cap, first.data(), &npasses, nullptr, 0) == ETHCNN_OK);
    int64_t groups = 0;
    for (int j = 0; j < n; ++j) {
        EXPECT(first[j] == groups);
        groups += (nctus[j] + 15) / 16;
    }
    const int64_t per = (cap ? cap : 131072) / 16;
    EXPECT(npasses == (groups + per - 1) / per);
    if (npasses < 0) return;
    std::vector<int> passes((size_t)npasses, -1);  // exactly npasses entries: a write behind them is the sanitizer's to find
    EXPECT(ethcnn_ldp_sessions_plan(nctus.data(), n, cap, nullptr, nullptr, passes.data(), npasses) == ETHCNN_OK);
    int64_t sum = 0;
    for (int p = 0; p < npasses; ++p) {
        EXPECT(passes[p] == std::min<int64_t>(per, groups - sum));
        EXPECT(passes[p] > 0 && (int64_t)passes[p] * 16 <= (cap ? cap : 131072));
        sum += passes[p];
    }
    EXPECT(sum == groups);
    if (npasses > 1) {  // fewer rows asked for than there are passes
        std::vector<int> head(1, -1);
        EXPECT(ethcnn_ldp_sessions_plan(nctus.data(), n, cap, nullptr, &npasses, head.data(), 1) == ETHCNN_OK && head[0] == passes[0]);
    }
}

int main() {
    const std::vector<int> counts = {1, 4, 12, 16, 17, 28, 1200};
    std::vector<std::vector<int>> orders = {counts, std::vector<int>(counts.rbegin(), counts.rend()), {1200, 1, 1200, 17, 16, 4, 12, 28, 1200}};
    std::vector<int> perm = counts;
    for (int k = 0; k < 12; ++k) {
        std::next_permutation(perm.begin(), perm.end());
        std::rotate(perm.begin(), perm.begin() + (k % 5) + 1, perm.end());
        orders.push_back(perm);
    }
    for (int c : counts) orders.push_back({c});
    orders.push_back(std::vector<int>(32, 1200));
    for (const auto& o : orders)
        for (int cap : {32, 0, 16, 1024}) check_plan(o, cap);

    const int two[2] = {4, 12}, zero[2] = {4, 0};
    int first[33], np = 0, pg[4];
    EXPECT(ethcnn_ldp_sessions_plan(zero, 2, 32, first, &np, pg, 4) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_ldp_sessions_plan(two, 0, 32, first, &np, pg, 4) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_ldp_sessions_plan(two, 33, 32, first, &np, pg, 4) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_ldp_sessions_plan(two, 2, 15, first, &np, pg, 4) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_ldp_sessions_plan(two, 2, -1, first, &np, pg, 4) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_ldp_sessions_plan(two, 2, 32, first, &np, nullptr, 4) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_ldp_sessions_plan(nullptr, 2, 32, first, &np, pg, 4) == ETHCNN_ERR_ARG);
    const std::vector<int> huge(32, INT32_MAX);  // the group total does not fit the ints of the table
    EXPECT(ethcnn_ldp_sessions_plan(huge.data(), 32, 0, first, &np, pg, 4) == ETHCNN_ERR_ARG);

    const int ws[6] = {72, 200, 1040, 416, 1, 2560}, hs[6] = {72, 136, 64, 240, 1, 1920};
    int64_t want = 0;
    for (int j = 0; j < 6; ++j) {
        const int64_t nctu = (int64_t)((ws[j] + 63) / 64) * ((hs[j] + 63) / 64);
        want += (nctu + 15) / 16 * 16 * (1792 + 3584);
    }
    EXPECT(ethcnn_ldp_sessions_bytes(ws, hs, 6) == want);
    EXPECT(ethcnn_ldp_sessions_bytes(ws, hs, 0) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_ldp_sessions_bytes(ws, hs, 33) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_ldp_sessions_bytes(nullptr, hs, 1) == ETHCNN_ERR_ARG);
    // a picture of more CTUs than a session can have is refused (no int overflow on the way); 32 of the largest accepted ones sum in int64
    const int big[2] = {INT32_MAX, INT32_MAX};
    EXPECT(ethcnn_ldp_sessions_bytes(big, big, 1) == ETHCNN_ERR_ARG);
    EXPECT(ethcnn_ldp_sessions_bytes(big, big, 2) == ETHCNN_ERR_ARG);
    const std::vector<int> wide(32, 64 * 8191), tall(32, 64 * 16383);
    const int64_t most = (int64_t)8191 * 16383;
    EXPECT(ethcnn_ldp_sessions_bytes(wide.data(), tall.data(), 32) == 32 * ((most + 15) / 16 * 16) * 5376);
    const int neg[1] = {-64};
    EXPECT(ethcnn_ldp_sessions_bytes(neg, hs, 1) == ETHCNN_ERR_ARG);
    std::printf("ldp_sessions_plan_check: %zu orders, %d failures\n", orders.size(), failures);
    return failures ? 1 : 0;
}
