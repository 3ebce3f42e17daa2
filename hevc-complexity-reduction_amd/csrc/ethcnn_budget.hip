// ethcnn_budget.hip -- the two kernels of the search budget (layouts and launch notes: ethcnn_budget.h; the contract: include/ethcnn.h
// "search budget").  k_budget_cost is k_sim_eval's scheme (ethcnn_sim.hip) with another ownership -- a wave owns 64 rungs and the CTUs
// of one frame -- and keeps the four `checked` counters only; k_budget_bake is k_decide's scheme (ethcnn_decide.hip) with the
// thresholds taken per frame and the outcome written as the 21 values an unchanged encoder reads.  The rule itself is shared with
// k_decide through ethcnn_node_masks.h.  Integers and bit masks only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ethcnn_budget.h"
#include "ethcnn_node_masks.h"
#include "ethcnn_sim.h"

namespace ethcnn {
namespace budget {

namespace {
using sim::kL1;
using sim::kL2;
using sim::kRecDwords;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr long kMaxBlocks = 1L << 30;
constexpr unsigned kOne = 0x3f800000u, kHalf = 0x3f000000u;  // 1.0f, 0.5f (0.0f is 0)

__global__ __launch_bounds__(kThreads) void k_budget_cost(const unsigned* __restrict__ recs, long per, long nframes, const int* __restrict__ thr,
                                                          int rungs, int rung_waves, int slices, long slice_len, unsigned* __restrict__ out) {
    const long wave = blockIdx.x * (long)kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long unit = wave / rung_waves;  // (frame, slice)
    const long frame = unit / slices;
    if (frame >= nframes) return;
    const long slice = unit - frame * slices;
    const int c = (int)(wave - unit * rung_waves) * 64 + (int)(threadIdx.x & 63);
    const bool live = c < rungs;
    const int* th = thr + (long)(live ? c : rungs - 1) * 6;
    const int up[3] = {th[0], th[1], th[2]}, down[3] = {th[3], th[4], th[5]};
    unsigned n64 = 0u, n32 = 0u, n16 = 0u, n8 = 0u;
    const long first = slice * slice_len, last = first + slice_len < per ? first + slice_len : per;
    const unsigned* r = recs + (frame * per + first) * kRecDwords;
    for (long i = first; i < last; ++i, r += kRecDwords) {
        unsigned w[14];  // the bins and the three geometry masks; truth and sub-batch are not needed
#pragma unroll
        for (int k = 0; k < 14; ++k) w[k] = r[k];
        unsigned so, le;
        sim::compare_bins(w, up, down, so, le);
        const sim::Descent ds = sim::descend(so, le, w[11], w[12]);
        const unsigned chk = ds.dec & ~so;  // CURRENT ONLY or BOTH: the CU itself is checked
        n64 += chk & 1u;
        n32 += __popc(chk & kL1);
        n16 += __popc(chk & kL2);
        // 8 x 8 CUs: four under a recursing 16 x 16 node, two (one in the corner) under an edge node
        n8 += 4u * __popc(ds.dec & ds.rec & kL2) + 2u * __popc(ds.edg & kL2) - __popc(ds.edg & w[13]);
    }
    if (!live) return;
    unsigned* o = out + (frame * rungs + c) * 4;
    if (n64) atomicAdd(&o[0], n64);
    if (n32) atomicAdd(&o[1], n32);
    if (n16) atomicAdd(&o[2], n16);
    if (n8) atomicAdd(&o[3], n8);
}

__global__ __launch_bounds__(kThreads) void k_budget_bake(const uint4* __restrict__ recs, long per, long ctu0, long n, const int* __restrict__ frame_thr,
                                                          unsigned* __restrict__ probs) {
    __shared__ unsigned s_rows[kThreads * kNout];
    const int t = threadIdx.x;
    const long base = (long)blockIdx.x * kThreads;
    const int cur = (int)(n - base < kThreads ? n - base : kThreads);
    if (t < cur) {
        const long ctu = ctu0 + base + t;  // its index in the window
        unsigned w[kRecDwords];
        {
            const uint4* r = recs + ctu * 4;
            const uint4 a = r[0], b = r[1], e = r[2], d = r[3];
            w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
            w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
            w[8] = e.x, w[9] = e.y, w[10] = e.z, w[11] = e.w;
            w[12] = d.x, w[13] = d.y, w[14] = d.z, w[15] = d.w;
        }
        const int* th = frame_thr + (ctu / per) * 6;
        const int up[3] = {th[0], th[1], th[2]}, down[3] = {th[3], th[4], th[5]};
        unsigned so, le;
        sim::compare_bins(w, up, down, so, le);
        const unsigned inside = w[11], edge = w[12];
        const sim::Descent ds = sim::descend(so, le, inside, edge);
        const bool live = ((inside | edge) & 1u) != 0u;  // a rejected CTU has empty masks: it gets the full search
        const unsigned one = live ? ds.d_so | ds.edg : 0u, half = live ? ds.d_bo : 0x1fffffu;
#pragma unroll
        for (int k = 0; k < kNout; ++k) s_rows[t * kNout + sim::raster_of(k)] = (one >> k & 1u) ? kOne : (half >> k & 1u) ? kHalf : 0u;
    }
    __syncthreads();
    unsigned* dst = probs + base * kNout;
#pragma unroll
    for (int i = 0; i < kNout; ++i) {
        const int at = t + kThreads * i;
        if (at < cur * kNout) dst[at] = s_rows[at];
    }
}
}  // namespace

void launch_cost(hipStream_t s, const unsigned* recs, long per, long nframes, const int* d_thr, int rungs, unsigned* d_checked, int cus) {
    if (per <= 0 || nframes <= 0 || rungs <= 0) return;
    // waves = rung groups x slices x frames: a frame is cut into slices (of at least 64 CTUs) only while there are fewer than about
    // 16 waves a CU
    const long rung_waves = (rungs + 63) / 64;
    long slices = (16L * cus + rung_waves * nframes - 1) / (rung_waves * nframes);
    slices = std::max(std::min(slices, (per + 63) / 64), 1L);
    const long slice_len = (per + slices - 1) / slices;
    slices = (per + slice_len - 1) / slice_len;
    const long per_frame = rung_waves * slices;  // waves
    const long chunk = std::max(1L, kMaxBlocks * kWaves / per_frame);  // frames a launch
    for (long f = 0; f < nframes; f += chunk) {
        const long m = std::min(chunk, nframes - f);
        const long blocks = (m * per_frame + kWaves - 1) / kWaves;
        k_budget_cost<<<(unsigned)blocks, kThreads, 0, s>>>(recs + f * per * kRecDwords, per, m, d_thr, rungs, (int)rung_waves, (int)slices, slice_len,
                                                            d_checked + f * rungs * 4);
    }
}

void launch_bake(hipStream_t s, const unsigned* recs, long per, long ctu0, long n, const int* d_frame_thr, float* d_probs) {
    if (per <= 0 || n <= 0) return;
    const long chunk = kMaxBlocks * kThreads;  // CTUs a launch
    for (long at = 0; at < n; at += chunk) {
        const long m = std::min(chunk, n - at);
        k_budget_bake<<<(unsigned)((m + kThreads - 1) / kThreads), kThreads, 0, s>>>(reinterpret_cast<const uint4*>(recs), per, ctu0 + at, m, d_frame_thr,
                                                                                   reinterpret_cast<unsigned*>(d_probs) + at * kNout);
    }
}

}  // namespace budget
}  // namespace ethcnn
