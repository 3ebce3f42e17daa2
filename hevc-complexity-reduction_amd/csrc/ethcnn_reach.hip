// ethcnn_reach.hip -- the kernel of the threshold calibration on reached nodes (shape and launch notes: ethcnn_reach.h; the definition:
// include/ethcnn.h "threshold calibration on reached nodes").  The rule on a record and the gates come from ethcnn_node_masks.h, as in
// every kernel of this family.  Integer counting only: the histogram is exact and independent of the schedule.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ethcnn_node_masks.h"
#include "ethcnn_reach.h"

namespace ethcnn {
namespace reach {

namespace {
constexpr int kThreads = 256;
constexpr int kBins = calib::kBins;

// Block (x, y) = (slice of the records, candidate); lane = record.  Unlabelled and rejected records add nothing (a rejected CTU
// carries no label bit).  Per labelled record: the masks of the candidate, the gates, the descent; then one LDS add per decided node,
// at the bin the encoder reads (0 where a closed gate zeroed it).  Real probabilities pile up in bins 0, 1 and 1024, so the adds of a
// wave often meet in a few words; the LDS atomic unit serialises those.  Measured (profiles/reach_rate.json): 1.8 times the time of
// uniform data at 16 candidates, 1.04 times at one; counting the hot bins with wave ballots first was tried and was slower on both.
__global__ __launch_bounds__(kThreads) void k_reach_hist(const uint4* __restrict__ recs, const unsigned* __restrict__ m, long n, const int* __restrict__ cand,
                                                         long slice_len, int gate_order, unsigned long long* __restrict__ out) {
    __shared__ unsigned s_hist[kHistWords];
    const int t = threadIdx.x;
    for (int i = t; i < kHistWords; i += kThreads) s_hist[i] = 0u;
    __syncthreads();
    const int* th = cand + (size_t)blockIdx.y * 6;  // (the same address in every lane: scalar loads)
    const int up[3] = {th[0], th[1], th[2]}, down[3] = {th[3], th[4], th[5]};
    int g1, g2;
    sim::gate_thresholds(gate_order, up, down, g1, g2);
    const long first = blockIdx.x * slice_len, last = first + slice_len < n ? first + slice_len : n;
    for (long i = first + t; i < last; i += kThreads) {
        const uint4 q3 = recs[i * 4 + 3];  // edge, corner, truth, sub-batch
        const unsigned truth = q3.z;
        if (!(truth >> 31)) continue;      // not labelled
        const uint4 q0 = recs[i * 4], q1 = recs[i * 4 + 1], q2 = recs[i * 4 + 2];
        const unsigned w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};  // 21 bins, the inside mask
        unsigned so, le;
        sim::compare_bins(w, up, down, so, le);
        const unsigned closed = sim::close_gates(m, q3.w, g1, g2, down, so, le);
        const unsigned dec = sim::descend(so, le, w[11], q3.x).dec;
#pragma unroll
        for (int k = 0; k < 21; ++k) {
            if (dec >> k & 1u) {
                unsigned bin = w[k >> 1] >> (16 * (k & 1)) & 0xffffu;
                bin = bin < (unsigned)(kBins - 1) ? bin : (unsigned)(kBins - 1);  // (k_sim_pack writes 0..1024: never outside the histogram)
                if (closed >> k & 1u) bin = 0u;
                const int l = k == 0 ? 0 : k < 5 ? 1 : 2;
                atomicAdd(&s_hist[(l * 2 + (int)(truth >> k & 1u)) * kBins + (int)bin], 1u);
            }
        }
    }
    __syncthreads();
    unsigned long long* o = out + (size_t)blockIdx.y * kHistWords;
    for (int i = t; i < kHistWords; i += kThreads) {
        const unsigned v = s_hist[i];
        if (v) atomicAdd(&o[i], (unsigned long long)v);
    }
}
}  // namespace

void launch_hist(hipStream_t s, const unsigned* recs, const unsigned* m, long n, const int* cand, long ncand, int gate_order, unsigned long long* out,
                 int cus) {
    if (n <= 0 || ncand <= 0) return;
    // blocks = candidates x slices: about 4 blocks a CU (a block flushes up to 6150 words), slices of at least one trip of the block and
    // at most kMaxSlice CTUs
    long slices = (4L * cus + ncand - 1) / ncand;
    slices = std::min(slices, (n + kThreads - 1) / kThreads);
    slices = std::max(std::max(slices, 1L), (n + kMaxSlice - 1) / kMaxSlice);
    const long slice_len = (n + slices - 1) / slices;
    slices = (n + slice_len - 1) / slice_len;
    k_reach_hist<<<dim3((unsigned)slices, (unsigned)ncand), kThreads, 0, s>>>(reinterpret_cast<const uint4*>(recs), m, n, cand, slice_len, gate_order, out);
}

}  // namespace reach
}  // namespace ethcnn
