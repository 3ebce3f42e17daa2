// ethcnn_ladder.cpp -- host side of the ladder search (include/ethcnn.h "search budget: building a ladder"): the build around
// k_ladder_step (ethcnn_ladder.hip) over a simulator's set, and the host-only argument rules, thinning and ladder file.
#include "ethcnn_ctx.h"
#include "ethcnn_budget.h"
#include "ethcnn_ladder.h"
#include "ethcnn_sim.h"

using namespace ethcnn::ladder;
using ethcnn::budget::kMaxRungs;

namespace {
typedef unsigned __int128 u128;
const uint64_t kDefaultWeight[4] = {64, 16, 4, 1};

int cus_of(const ethcnn_ctx* c) { return c->cus > 0 ? c->cus : 256; }

// the rules of the four plain arguments; c may be NULL (the message then goes where ethcnn_last_error(NULL) reads)
int check_rules(ethcnn_ctx* c, const uint64_t* weight, int grid, int64_t max_rungs, uint32_t max_bad_ppm) {
    if (weight)
        for (int d = 0; d < 4; ++d)
            if (weight[d] >> 32) return set_err(c, ETHCNN_ERR_ARG, "weight[%d] = %llu is not below 2^32", d, (unsigned long long)weight[d]);
    if (grid < 1 || grid > 1024 || (grid & (grid - 1))) return set_err(c, ETHCNN_ERR_ARG, "the grid is a power of two in 1..1024: got %d", grid);
    if (max_rungs < 1 || max_rungs > kMaxRungs) return set_err(c, ETHCNN_ERR_ARG, "a ladder has 1..%d rungs: got max_rungs = %lld", kMaxRungs, (long long)max_rungs);
    if (max_bad_ppm > 1000000u) return set_err(c, ETHCNN_ERR_ARG, "the share of bad CTUs is in parts per million, 0..1000000: got %u", max_bad_ppm);
    return 0;
}
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
    const uint64_t* w = weight ? weight : kDefaultWeight;
    // a CTU has at most 1, 4, 16 and 64 checked CUs of the four sizes: the largest cost any rung can have on this set
    const u128 bound = (u128)k->ctus * ((u128)w[0] + (u128)4 * w[1] + (u128)16 * w[2] + (u128)64 * w[3]);
    if (bound >> 64) return set_err(c, ETHCNN_ERR_ARG, "the cost of a set of %lld CTUs may not fit in 64 bits under these weights", (long long)k->ctus);

    // rung 0, the full search, by the simulator's own evaluation
    std::vector<ethcnn_ladder_rung> rungs((size_t)max_rungs);
    std::memset(rungs.data(), 0, rungs.size() * sizeof rungs[0]);
    ethcnn_ladder_rung& r0 = rungs[0];
    r0.thr = ethcnn_sim_thr{{1024, 1024, 1024}, {-1, -1, -1}};
    r0.coord = -1;
    r0.value = 0;
    ethcnn_sim_counts full;
    if (int rc = ethcnn_sim_eval(k, &r0.thr, 1, ETHCNN_SIM_GATES_NONE, &full)) return rc;
    unsigned long long st[kStateWords] = {0};
    for (int d = 0; d < 4; ++d) {
        r0.checked[d] = full.checked[d];
        st[kStateCost] += w[d] * full.checked[d];
    }
    r0.bad_ctus = full.bad_ctus;
    st[kStateBad] = full.bad_ctus;
    st[kStateRungs] = 1;
    st[kStateDone] = max_rungs == 1;
    for (int l = 0; l < 3; ++l) st[kStateUp + l] = 1024ull, st[kStateDown + l] = (unsigned long long)-1ll;

    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;  // the context's completion word does not cover these launches
    const int slots = slots_of(grid);
    const size_t table_bytes = (size_t)6 * slots * kTableFields * 8, state_bytes = kStateWords * 8, rung_bytes = (size_t)max_rungs * sizeof(ethcnn_ladder_rung);
    uint8_t* d = nullptr;  // table, state, rungs: one allocation, each part 8-byte aligned
    if (hipMalloc((void**)&d, table_bytes + state_bytes + rung_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, ETHCNN_ERR_NOMEM, "ladder search: %llu bytes of table, state and rungs do not fit in device memory",
                       (unsigned long long)(table_bytes + state_bytes + rung_bytes));
    }
    StepArgs a;
    a.recs = k->d_recs;
    a.n = (long)k->ctus;
    a.table = reinterpret_cast<unsigned long long*>(d);
    a.state = reinterpret_cast<unsigned long long*>(d + table_bytes);
    a.rungs = reinterpret_cast<ethcnn_ladder_rung*>(d + table_bytes + state_bytes);
    for (int i = 0; i < 4; ++i) a.weight[i] = w[i];
    a.cap = (unsigned long long)max_bad_ppm * k->labelled;  // (labelled CTUs lie in HBM: far below 2^44)
    a.grid = grid;
    a.slots = slots;
    a.values = values_of(grid);
    a.max_rungs = (int)max_rungs;

    hipError_t e = hipMemsetAsync(d, 0, table_bytes, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(a.state, st, state_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(a.rungs, &r0, sizeof r0, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    // steps in batches: a step that finds the done flag set exits at once, so a batch may run past the end of the walk
    while (e == hipSuccess && !st[kStateDone]) {
        const int64_t left = max_rungs - (int64_t)st[kStateRungs];
        for (int64_t i = 0; i < std::min<int64_t>(kBatch, left); ++i) launch_step(c->stream, a, cus_of(c));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(st, a.state, state_bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess && !st[kStateDone] && (int64_t)st[kStateRungs] + left <= max_rungs) {  // every step appends a rung or sets the flag
            (void)hipFree(d);
            return set_err(c, ETHCNN_ERR_DEVICE, "ladder search: a batch of steps left the walk at %llu rungs without ending it", st[kStateRungs]);
        }
    }
    const int64_t n = (int64_t)st[kStateRungs];
    if (e == hipSuccess && (n < 1 || n > max_rungs || st[kStateTicket])) {
        (void)hipFree(d);
        return set_err(c, ETHCNN_ERR_DEVICE, "ladder search: the state block came back with %lld rungs and ticket %llu", (long long)n, st[kStateTicket]);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(rungs.data(), a.rungs, (size_t)n * sizeof(ethcnn_ladder_rung), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, ETHCNN_ERR_DEVICE, "ladder search: %s", hipGetErrorString(e));
    }
    std::memcpy(rungs_out, rungs.data(), (size_t)n * sizeof(ethcnn_ladder_rung));
    *nrungs_out = n;
    return ETHCNN_OK;
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
    if (K < 1 || K > kMaxRungs) return set_err(nullptr, ETHCNN_ERR_ARG, "a ladder has 1..%d rungs: got %lld", kMaxRungs, (long long)K);
    for (int64_t i = 0; i < K; ++i)
        if (int rc = ethcnn::sim::check_cand(nullptr, thr[i], (long long)i)) return rc;
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long)getpid());  // never a partial ladder file
    FILE* f = std::fopen(tmp.c_str(), "w");
    if (!f) return set_err(nullptr, ETHCNN_ERR_IO, "cannot open %s for writing: %s", tmp.c_str(), std::strerror(errno));
    int rc = 0;
    for (int64_t i = 0; i < K && !rc; ++i) {
        double v[6];
        for (int l = 0; l < 3; ++l) {
            v[2 * l + (order == ETHCNN_THR_ORDER_AI ? 1 : 0)] = thr[i].down_k[l] / 1024.0;
            v[2 * l + (order == ETHCNN_THR_ORDER_AI ? 0 : 1)] = thr[i].up_k[l] / 1024.0;
        }
        if (std::fprintf(f, "%.10f %.10f %.10f %.10f %.10f %.10f\n", v[0], v[1], v[2], v[3], v[4], v[5]) < 0)
            rc = set_err(nullptr, ETHCNN_ERR_IO, "write to %s failed: %s", tmp.c_str(), std::strerror(errno));
    }
    if (std::fclose(f) != 0 && !rc) rc = set_err(nullptr, ETHCNN_ERR_IO, "close of %s failed", tmp.c_str());
    if (!rc && std::rename(tmp.c_str(), path) != 0) rc = set_err(nullptr, ETHCNN_ERR_IO, "rename %s -> %s failed: %s", tmp.c_str(), path, std::strerror(errno));
    if (rc) std::remove(tmp.c_str());
    return rc;
}
