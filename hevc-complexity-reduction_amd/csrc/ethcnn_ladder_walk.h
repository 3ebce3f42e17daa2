// ethcnn_ladder_walk.h -- host only: the greedy ladder walk over a simulator's set, once for the two kernels that step it (the host
// side of ethcnn_ladder_step.h).  What the two walks differ in comes from a host-side kind K:
//   K::Args, K::Rung          the launch arguments and the rung record of the kernel's kind
//   K::kTableFields           uint64 words of a table row
//   K::launch(s, a, cus)      one step
//   k.rung0(sim, full, r0, harm)   the kind's own fields of rung 0, the full search whose counters are `full`, and what the state word
//                             kStateBad holds for it; 0 or an error code
//   k.fill(a, sim)            the kind's own launch arguments (the cap)
#pragma once
#include "ethcnn_analysis.h"
#include "ethcnn_ladder.h"

namespace ethcnn {
namespace ladder {

// checked arguments -> rungs_out[0 .. *nrungs_out), both untouched on failure
template <class K>
int walk(ethcnn_sim* k, const K& kind, const uint64_t* weight, int grid, int64_t max_rungs, typename K::Rung* rungs_out, int64_t* nrungs_out) {
    typedef typename K::Rung Rung;
    ethcnn_ctx* c = k->c;
    const uint64_t* w = weight ? weight : sim::kDefaultWeight;
    if (!sim::cost_fits(k->ctus, w)) return set_err(c, ETHCNN_ERR_ARG, "the cost of a set of %lld CTUs may not fit in 64 bits under these weights", (long long)k->ctus);

    // rung 0, the full search, by the simulator's own evaluation
    std::vector<Rung> rungs((size_t)max_rungs);
    std::memset(rungs.data(), 0, rungs.size() * sizeof rungs[0]);
    Rung& r0 = rungs[0];
    r0.thr = sim::kFullSearch;
    r0.coord = -1;
    r0.value = 0;
    ethcnn_sim_counts full;
    if (int rc = ethcnn_sim_eval(k, &r0.thr, 1, ETHCNN_SIM_GATES_NONE, &full)) return rc;
    unsigned long long st[kStateWords] = {0};
    if (int rc = kind.rung0(k, full, r0, &st[kStateBad])) return rc;
    for (int d = 0; d < 4; ++d) {
        r0.checked[d] = full.checked[d];
        st[kStateCost] += w[d] * full.checked[d];
    }
    st[kStateRungs] = 1;
    st[kStateDone] = max_rungs == 1;
    for (int l = 0; l < 3; ++l) st[kStateUp + l] = 1024ull, st[kStateDown + l] = (unsigned long long)-1ll;

    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;  // the context's completion word does not cover these launches
    const int slots = slots_of(grid);
    const size_t table_bytes = (size_t)6 * slots * K::kTableFields * 8, state_bytes = kStateWords * 8, rung_bytes = (size_t)max_rungs * sizeof(Rung);
    Scratch d;  // table, state, rungs: one allocation, each part 8-byte aligned
    if (int rc = d.alloc(c, table_bytes + state_bytes + rung_bytes, "ladder search")) return rc;
    typename K::Args a;
    a.recs = k->d_recs;
    a.n = (long)k->ctus;
    a.table = d.at<unsigned long long>();
    a.state = d.at<unsigned long long>(table_bytes);
    a.rungs = d.at<Rung>(table_bytes + state_bytes);
    for (int i = 0; i < 4; ++i) a.weight[i] = w[i];
    a.grid = grid;
    a.slots = slots;
    a.values = values_of(grid);
    a.max_rungs = (int)max_rungs;
    kind.fill(a, k);

    hipError_t e = hipMemsetAsync(a.table, 0, table_bytes, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(a.state, st, state_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(a.rungs, &r0, sizeof r0, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    // steps in batches: a step that finds the done flag set exits at once, so a batch may run past the end of the walk
    while (e == hipSuccess && !st[kStateDone]) {
        const int64_t left = max_rungs - (int64_t)st[kStateRungs];
        for (int64_t i = 0; i < std::min<int64_t>(kBatch, left); ++i) K::launch(c->stream, a, cus_of(c));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(st, a.state, state_bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess && !st[kStateDone] && (int64_t)st[kStateRungs] + left <= max_rungs)  // every step appends a rung or sets the flag
            return set_err(c, ETHCNN_ERR_DEVICE, "ladder search: a batch of steps left the walk at %llu rungs without ending it", st[kStateRungs]);
    }
    const int64_t n = (int64_t)st[kStateRungs];
    if (e == hipSuccess && (n < 1 || n > max_rungs || st[kStateTicket]))
        return set_err(c, ETHCNN_ERR_DEVICE, "ladder search: the state block came back with %lld rungs and ticket %llu", (long long)n, st[kStateTicket]);
    if (e == hipSuccess) e = hipMemcpyAsync(rungs.data(), a.rungs, (size_t)n * sizeof(Rung), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, ETHCNN_ERR_DEVICE, "ladder search: %s", hipGetErrorString(e));
    }
    std::memcpy(rungs_out, rungs.data(), (size_t)n * sizeof(Rung));
    *nrungs_out = n;
    return ETHCNN_OK;
}

}  // namespace ladder
}  // namespace ethcnn
