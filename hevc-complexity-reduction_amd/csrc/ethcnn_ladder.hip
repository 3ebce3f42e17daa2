// ethcnn_ladder.hip -- the kernel of the ladder search (layouts and launch notes: ethcnn_ladder.h; the rule: include/ethcnn.h "search
// budget: building a ladder").  k_ladder_step is one step of the greedy walk in one launch: every single-coordinate move from the
// current rung is evaluated over the simulator's records, and the block that draws the last ticket picks one and appends the rung.  The
// step itself is ethcnn_ladder_step.h, shared with the walk by expected wrong decisions (ethcnn_risk.hip); here is what the labelled
// walk adds to it.  The rule on a record is shared with k_decide, k_budget_* and k_pacer_frame through ethcnn_node_masks.h.
#include <hip/hip_runtime.h>

#include "../../include/ethcnn.h"
#include "ethcnn_ladder.h"
#include "ethcnn_ladder_step.h"

namespace ethcnn {
namespace ladder {

namespace {
// the labelled kind of ethcnn_ladder_step.h: a move is weighed by the bad CTUs it leaves
struct Labelled {
    typedef StepArgs Args;
    typedef ethcnn_ladder_rung Rung;
    static constexpr int kFields = kTableFields;
    struct Count {
        unsigned nbad = 0u;
        __device__ __forceinline__ void record(const Args&, const unsigned* w, const sim::Descent& ds) {
            const unsigned truth = w[14], t_split = truth & 0x1fffffu, t_unsplit = (truth >> 31 ? ~truth : 0u) & 0x1fffffu;
            nbad += ((ds.d_so & t_unsplit) | (ds.d_co & t_split)) ? 1u : 0u;
        }
        __device__ __forceinline__ void flush(u64* o) const {
            if (nbad) __hip_atomic_fetch_add(&o[4], (u64)nbad, LADDER_AGENT);
        }
    };
    static __device__ __forceinline__ u64 harm(const u64* row) { return __hip_atomic_load(row + 4, LADDER_AGENT); }
    static __device__ __forceinline__ bool over_cap(const Args& a, u64 bad) { return (u128)bad * 1000000u > (u128)a.cap; }
    static __device__ __forceinline__ void finish(Rung& rung, const u64* row) { rung.bad_ctus = harm(row); }
};

__global__ __launch_bounds__(kThreads) void k_ladder_step(const unsigned* __restrict__ recs, const StepArgs a, const int coord_waves, const long slices,
                                                          const long slice_len) {
    step<Labelled>(recs, a, coord_waves, slices, slice_len);
}
}  // namespace

void launch_step(hipStream_t s, const StepArgs& a, int cus) {
    if (a.n <= 0) return;
    int coord_waves;
    long slices, slice_len;
    const long blocks = step_shape(a.n, a.values, cus, &coord_waves, &slices, &slice_len);
    k_ladder_step<<<(unsigned)blocks, kThreads, 0, s>>>(a.recs, a, coord_waves, slices, slice_len);
}

}  // namespace ladder
}  // namespace ethcnn
