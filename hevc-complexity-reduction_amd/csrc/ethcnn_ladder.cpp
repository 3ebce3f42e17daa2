// ethcnn_ladder.cpp -- host side of the ladder search (include/ethcnn.h "search budget: building a ladder"): the build around
// k_ladder_step (ethcnn_ladder.hip) over a simulator's set, and the host-only argument rules, thinning and ladder file.
#include "ethcnn_ctx.h"
#include "ethcnn_ladder.h"
#include "ethcnn_ladder_walk.h"

using namespace ethcnn::ladder;

namespace {
// the rules of the four plain arguments; c may be NULL (the message then goes where ethcnn_last_error(NULL) reads)
int check_rules(ethcnn_ctx* c, const uint64_t* weight, int grid, int64_t max_rungs, uint32_t max_bad_ppm) {
    if (int rc = sim::check_weights(c, weight)) return rc;
    if (grid < 1 || grid > 1024 || (grid & (grid - 1))) return set_err(c, ETHCNN_ERR_ARG, "the grid is a power of two in 1..1024: got %d", grid);
    if (int rc = sim::check_rung_count(c, max_rungs, "", "max_rungs = ")) return rc;
    if (max_bad_ppm > 1000000u) return set_err(c, ETHCNN_ERR_ARG, "the share of bad CTUs is in parts per million, 0..1000000: got %u", max_bad_ppm);
    return 0;
}

// the walk's kind for k_ladder_step: a move is weighed by the newly bad CTUs
struct ByLabels {
    typedef StepArgs Args;
    typedef ethcnn_ladder_rung Rung;
    static constexpr int kTableFields = ethcnn::ladder::kTableFields;
    uint32_t max_bad_ppm;
    static void launch(hipStream_t s, const Args& a, int cus) { launch_step(s, a, cus); }
    int rung0(ethcnn_sim*, const ethcnn_sim_counts& full, Rung& r0, unsigned long long* harm) const {
        *harm = r0.bad_ctus = full.bad_ctus;
        return 0;
    }
    void fill(Args& a, const ethcnn_sim* k) const { a.cap = (unsigned long long)max_bad_ppm * k->labelled; }  // (labelled CTUs lie in HBM: far below 2^44)
};
}  // namespace

extern "C" int ethcnn_ladder_check(const uint64_t weight[4], int grid, int64_t max_rungs, uint32_t max_bad_ppm) {
    return check_rules(nullptr, weight, grid, max_rungs, max_bad_ppm);
}

extern "C" int ethcnn_ladder_build(ethcnn_sim* k, const uint64_t weight[4], int grid, int64_t max_rungs, uint32_t max_bad_ppm, ethcnn_ladder_rung* rungs_out,
                                   int64_t* nrungs_out) {
    static_assert(sizeof(ethcnn_ladder_rung) == 72, "the kernel writes this layout");
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (!rungs_out || !nrungs_out) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ladder_build: null output");
    if (int rc = check_rules(c, weight, grid, max_rungs, max_bad_ppm)) return rc;
    if (k->labelled == 0) return set_err(c, ETHCNN_ERR_ARG, "a ladder is built from labelled CTUs: the set holds none");
    return walk(k, ByLabels{max_bad_ppm}, weight, grid, max_rungs, rungs_out, nrungs_out);
}

extern "C" int ethcnn_ladder_thin(const uint64_t* cost, int64_t n, int64_t K, int32_t* idx_out, int64_t* k_out) {
    if (!cost || !idx_out || !k_out) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_ladder_thin: null argument");
    if (n < 1 || K < 1 || n > INT32_MAX) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_ladder_thin: n = %lld, K = %lld (both at least 1)", (long long)n, (long long)K);
    for (int64_t i = 1; i < n; ++i)
        if (cost[i] >= cost[i - 1])
            return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_ladder_thin: the costs fall strictly along a ladder: cost[%lld] = %llu after %llu", (long long)i,
                           (unsigned long long)cost[i], (unsigned long long)cost[i - 1]);
    if (n <= K) {
        for (int64_t i = 0; i < n; ++i) idx_out[i] = (int32_t)i;
        *k_out = n;
        return ETHCNN_OK;
    }
    int64_t count = 0, i = 0;
    const uint64_t span = cost[0] - cost[n - 1];
    for (int64_t j = 0; j < K; ++j) {
        const uint64_t target = K == 1 ? cost[0] : cost[0] - (uint64_t)((u128)(uint64_t)j * span / (uint64_t)(K - 1));
        while (cost[i] > target) ++i;  // (targets fall with j, and cost[n - 1] <= every target)
        if (count == 0 || idx_out[count - 1] != (int32_t)i) idx_out[count++] = (int32_t)i;
    }
    *k_out = count;
    return ETHCNN_OK;
}

extern "C" int ethcnn_ladder_write(const char* path, const ethcnn_sim_thr* thr, int64_t K, int order) {
    if (!path || !thr) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_ladder_write: null argument");
    if (order != ETHCNN_THR_ORDER_AI && order != ETHCNN_THR_ORDER_LDP)
        return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_ladder_write: order %d is neither ETHCNN_THR_ORDER_AI nor ETHCNN_THR_ORDER_LDP", order);
    if (int rc = sim::check_rung_count(nullptr, K)) return rc;
    std::string text;
    for (int64_t i = 0; i < K; ++i) {
        if (int rc = sim::check_cand(nullptr, thr[i], (long long)i)) return rc;
        text += thr_line(thr[i].down_k, thr[i].up_k, order);
    }
    return write_text_atomic(path, text);
}
