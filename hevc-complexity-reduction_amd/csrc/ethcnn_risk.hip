// ethcnn_risk.hip -- the two kernels of the expected wrong decisions (layouts and launch notes: ethcnn_risk.h; the definition:
// include/ethcnn.h "partition-search simulation: expected wrong decisions").  k_sim_risk scores candidates, k_ladder_step_risk is the
// ladder walk's step weighed by that score (the step itself: ethcnn_ladder_step.h).  The rule on a record comes from
// ethcnn_node_masks.h, as in every kernel of this family.  Integers only: the sums are exact and independent of the schedule.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ethcnn.h"
#include "ethcnn_ladder_step.h"
#include "ethcnn_risk.h"

namespace ethcnn {
namespace risk {

namespace {
using ladder::u128;
using ladder::u64;
constexpr int kThreads = ladder::kThreads;

// One record under one candidate: the table values of its 21 nodes, picked by the masks of the decided nodes that came out CURRENT
// ONLY (-> stop[level]) and SPLIT ONLY (-> split[level], the complement to kOne).  Bins and table values are the same in every lane;
// a lane's own part is one bit of each mask per node, which selects by a 24-bit multiply with 0 or 1 (values are at most 2^20; the
// compiler lowers it to a sign-extending one-bit extract and an AND).
struct Sums {
    unsigned split[3], stop[3];
};

__device__ __forceinline__ Sums sums_of(const unsigned* w, const unsigned* __restrict__ rel, unsigned d_so, unsigned d_co) {
    Sums s = {{0u, 0u, 0u}, {0u, 0u, 0u}};
#pragma unroll
    for (int k = 0; k < 21; ++k) {
        unsigned bin = w[k >> 1] >> (16 * (k & 1)) & 0xffffu;
        bin = bin < (unsigned)(kBins - 1) ? bin : (unsigned)(kBins - 1);  // (k_sim_pack writes 0..1024: the table is never read outside)
        const int l = k == 0 ? 0 : k < 5 ? 1 : 2;
        const unsigned r = rel[l * kBins + bin];
        s.stop[l] += __umul24(d_co >> k & 1u, r);
        s.split[l] += __umul24(d_so >> k & 1u, kOne - r);
    }
    return s;
}

__global__ __launch_bounds__(kThreads) void k_sim_risk(const unsigned* __restrict__ recs, long n, const int* __restrict__ cand, long ncand, int cand_waves,
                                                       long slices, long slice_len, const unsigned* __restrict__ rel, unsigned long long* __restrict__ out) {
    const long wave = blockIdx.x * (long)(kThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long slice = wave / cand_waves;
    if (slice >= slices) return;
    const long c = (wave - slice * cand_waves) * 64 + (threadIdx.x & 63);
    const bool live = c < ncand;
    const int* th = cand + (live ? c : ncand - 1) * 6;
    const int up[3] = {th[0], th[1], th[2]}, down[3] = {th[3], th[4], th[5]};
    u64 acc[kFields] = {0, 0, 0, 0, 0, 0};
    const long first = slice * slice_len, last = first + slice_len < n ? first + slice_len : n;
    for (long i = first; i < last; ++i) {
        const unsigned* r = recs + i * sim::kRecDwords;
        unsigned w[13];
#pragma unroll
        for (int k = 0; k < 13; ++k) w[k] = r[k];
        unsigned so, le;
        sim::compare_bins(w, up, down, so, le);
        const sim::Descent ds = sim::descend(so, le, w[11], w[12]);
        const Sums s = sums_of(w, rel, ds.d_so, ds.d_co);
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            acc[l] += s.split[l];
            acc[3 + l] += s.stop[l];
        }
    }
    if (!live) return;
    unsigned long long* o = out + c * kFields;
#pragma unroll
    for (int f = 0; f < kFields; ++f)
        if (acc[f]) atomicAdd(&o[f], acc[f]);
}

// the kind of ethcnn_ladder_step.h that weighs a move by the expected wrong decisions it leaves
struct Risk {
    typedef StepArgs Args;
    typedef ethcnn_ladder_rung_risk Rung;
    static constexpr int kFields = kTableFields;
    struct Count {
        u64 acc[risk::kFields] = {0, 0, 0, 0, 0, 0};
        __device__ __forceinline__ void record(const Args& a, const unsigned* w, const sim::Descent& ds) {
            const Sums s = sums_of(w, a.rel, ds.d_so, ds.d_co);
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                acc[l] += s.split[l];
                acc[3 + l] += s.stop[l];
            }
        }
        __device__ __forceinline__ void flush(u64* o) const {
#pragma unroll
            for (int f = 0; f < risk::kFields; ++f)
                if (acc[f]) __hip_atomic_fetch_add(&o[4 + f], acc[f], LADDER_AGENT);
        }
    };
    static __device__ __forceinline__ u64 harm(const u64* row) {
        u64 x = 0;
#pragma unroll
        for (int f = 0; f < risk::kFields; ++f) x += __hip_atomic_load(row + 4 + f, LADDER_AGENT);
        return x;
    }
    static __device__ __forceinline__ bool over_cap(const Args& a, u64 risk) { return (u128)risk * 1000000u > ((u128)a.cap_hi << 64 | (u128)a.cap_lo); }
    static __device__ __forceinline__ void finish(Rung& rung, const u64* row) {
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            rung.exp_wrong_split[l] = __hip_atomic_load(row + 4 + l, LADDER_AGENT);
            rung.exp_wrong_stop[l] = __hip_atomic_load(row + 7 + l, LADDER_AGENT);
        }
    }
};

__global__ __launch_bounds__(kThreads) void k_ladder_step_risk(const unsigned* __restrict__ recs, const StepArgs a, const int coord_waves, const long slices,
                                                               const long slice_len) {
    ladder::step<Risk>(recs, a, coord_waves, slices, slice_len);
}
}  // namespace

void launch_risk(hipStream_t s, const unsigned* recs, long n, const int* cand, long ncand, const unsigned* rel, unsigned long long* out, int cus) {
    if (n <= 0 || ncand <= 0) return;
    // waves = candidate groups x slices, sized as k_sim_eval's; a slice of at most kMaxSlice CTUs adds below 2^24 * 2^24 to a word
    const long cand_waves = (ncand + 63) / 64;
    long slices = (16L * cus + cand_waves - 1) / cand_waves;
    slices = std::min(slices, (n + 63) / 64);
    slices = std::max(std::max(slices, 1L), (n + sim::kMaxSlice - 1) / sim::kMaxSlice);
    const long slice_len = (n + slices - 1) / slices;
    slices = (n + slice_len - 1) / slice_len;
    const long blocks = (cand_waves * slices + kThreads / 64 - 1) / (kThreads / 64);
    k_sim_risk<<<(unsigned)blocks, kThreads, 0, s>>>(recs, n, cand, ncand, (int)cand_waves, slices, slice_len, rel, out);
}

void launch_step(hipStream_t s, const StepArgs& a, int cus) {
    if (a.n <= 0) return;
    int coord_waves;
    long slices, slice_len;
    const long blocks = ladder::step_shape(a.n, a.values, cus, &coord_waves, &slices, &slice_len);
    k_ladder_step_risk<<<(unsigned)blocks, kThreads, 0, s>>>(a.recs, a, coord_waves, slices, slice_len);
}

}  // namespace risk
}  // namespace ethcnn
