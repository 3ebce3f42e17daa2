// ethcnn_pacer.hip -- the kernel of the online search budget (layouts and launch notes: ethcnn_pacer.h; the contract: include/ethcnn.h
// "search budget, online").  k_pacer_frame is k_sim_pack + k_budget_cost + ethcnn_budget_choose of ONE frame in one launch: the frame's
// records never leave LDS between the pack and the count, and the block that draws the last ticket makes the choice.  The rule on a
// record is shared with k_decide and k_budget_* through ethcnn_node_masks.h.  Integers and bit masks only.
//
// The packing arithmetic is k_sim_pack's (ethcnn_sim.hip), RESTATED here rather than shared through a device function: k_sim_pack
// keeps labels, sub-batches and the M1 / M2 reduction in the same loop, and moving its body would not leave its ISA as it is.
#include <hip/hip_runtime.h>

#include "ethcnn_spec.h"
#include "ethcnn_node_masks.h"
#include "ethcnn_pacer.h"
#include "ethcnn_sim.h"

namespace ethcnn {
namespace pacer {

namespace {
using sim::kL1;
using sim::kL2;
using sim::kRecDwords;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kNout = 21;
typedef unsigned __int128 u128;
typedef unsigned long long u64;

#define PACER_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// one CTU: 21 probabilities in raster order -> its record (truth = 0, sub-batch = 0); rw x rh is the part of the CTU inside the picture
__device__ __forceinline__ void pack_ctu(const float* p, int rw, int rh, unsigned* w) {
#pragma unroll
    for (int i = 0; i < kRecDwords; ++i) w[i] = 0u;
    unsigned inside = 0u, edge = 0u, corner = 0u;
    bool rejected = false;
#pragma unroll
    for (int k = 0; k < kNout; ++k) {
        // node k: its raster index among the 21 probabilities and its square inside the CTU
        const int q = k - 5, j = k < 5 ? k - 1 : q >> 2, i = q & 3;
        const int bx = k == 0 ? 0 : k < 5 ? j & 1 : 2 * (j & 1) + (i & 1), by = k == 0 ? 0 : k < 5 ? j >> 1 : 2 * (j >> 1) + (i >> 1);
        const int s = k == 0 ? 64 : k < 5 ? 32 : 16, ox = bx * s, oy = by * s;
        const int r = k == 0 ? 0 : k < 5 ? 1 + bx + 2 * by : 5 + bx + 4 * by;
        const float v = p[r];
        const unsigned bits = __float_as_uint(v);
        if (bits > 0x3f800000u && bits != 0x80000000u) rejected = true;  // NaN, below 0, above 1 (-0 is 0)
        int bin = (int)ceilf(v * 1024.f);                                // exact product, 0..1024
        if (bin == 0 && (bits & 0x7fffffffu)) bin = 1;                   // p > 0 never lands in bin 0, whatever the denormal mode
        bin = bin < 0 ? 0 : bin > 1024 ? 1024 : bin;                     // (a rejected CTU's bins are never used)
        w[k >> 1] |= (unsigned)bin << (16 * (k & 1));
        if (ox + s <= rw && oy + s <= rh) inside |= 1u << k;
        else if (ox < rw && oy < rh) {
            edge |= 1u << k;
            if (k >= 5 && rw - ox < 16 && rh - oy < 16) corner |= 1u << k;
        }
    }
    if (rejected) inside = edge = corner = 0u;
    w[11] = inside;
    w[12] = edge;
    w[13] = corner;
}

__device__ __forceinline__ u64 load64(const unsigned* p) {
    return (u64)__hip_atomic_load(p, PACER_AGENT) | (u64)__hip_atomic_load(p + 1, PACER_AGENT) << 32;
}
__device__ __forceinline__ void store64(unsigned* p, u64 v) {
    __hip_atomic_store(p, (unsigned)v, PACER_AGENT);
    __hip_atomic_store(p + 1, (unsigned)(v >> 32), PACER_AGENT);
}

__global__ __launch_bounds__(kThreads) void k_pacer_frame(const FrameArgs a, const int rung_blocks, const int slice_len) {
    __shared__ uint4 s_rec[kSliceCtus * 4];
    __shared__ float s_p[kSliceCtus * kNout];
    __shared__ u64 s_cost[kWaves];
    __shared__ int s_fit[kWaves], s_least[kWaves];
    __shared__ int s_last;
    const int t = threadIdx.x;
    const int slice = (int)(blockIdx.x / (unsigned)rung_blocks), rb = (int)(blockIdx.x - (unsigned)slice * (unsigned)rung_blocks);
    const int first = slice * slice_len;
    const int cur = a.per - first < slice_len ? a.per - first : slice_len;  // 1..kSliceCtus

    // ---- pack: the slice's probabilities through LDS (coalesced), a lane per CTU
    {
        const float* src = a.probs + (long)first * kNout;
        for (int i = t; i < cur * kNout; i += kThreads) s_p[i] = src[i];
    }
    __syncthreads();
    if (t < cur) {
        const int ctu = first + t, cy = ctu / a.ctus_w, cx = ctu - cy * a.ctus_w;
        const int rw = a.width - 64 * cx < 64 ? a.width - 64 * cx : 64, rh = a.height - 64 * cy < 64 ? a.height - 64 * cy : 64;
        unsigned w[kRecDwords];
        pack_ctu(s_p + t * kNout, rw, rh, w);
        s_rec[t * 4 + 0] = make_uint4(w[0], w[1], w[2], w[3]);
        s_rec[t * 4 + 1] = make_uint4(w[4], w[5], w[6], w[7]);
        s_rec[t * 4 + 2] = make_uint4(w[8], w[9], w[10], w[11]);
        s_rec[t * 4 + 3] = make_uint4(w[12], w[13], w[14], w[15]);
    }
    __syncthreads();
    if (rb == 0) {  // one rung group of the slice keeps the records for the bake
        uint4* dst = reinterpret_cast<uint4*>(a.recs) + (long)first * 4;
        if (t < cur * 4) dst[t] = s_rec[t];
    }

    // ---- count: a lane is a rung, the wave walks the slice's records (every lane reads the same LDS address)
    {
        const int c = (rb * kWaves + (t >> 6)) * 64 + (t & 63);
        const bool live = c < a.rungs;
        const int* th = a.thr + (long)(live ? c : a.rungs - 1) * 6;
        const int up[3] = {th[0], th[1], th[2]}, down[3] = {th[3], th[4], th[5]};
        unsigned n64 = 0u, n32 = 0u, n16 = 0u, n8 = 0u;
        for (int i = 0; i < cur; ++i) {
            const uint4 r0 = s_rec[i * 4], r1 = s_rec[i * 4 + 1], r2 = s_rec[i * 4 + 2], r3 = s_rec[i * 4 + 3];
            const unsigned w[14] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y};
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
        if (live) {
            unsigned* o = a.checked + (long)c * 4;
            if (n64) __hip_atomic_fetch_add(&o[0], n64, PACER_AGENT);
            if (n32) __hip_atomic_fetch_add(&o[1], n32, PACER_AGENT);
            if (n16) __hip_atomic_fetch_add(&o[2], n16, PACER_AGENT);
            if (n8) __hip_atomic_fetch_add(&o[3], n8, PACER_AGENT);
        }
    }

    // ---- ticket: every wave's adds and stores are performed, then one lane releases and draws; nobody waits for anybody
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(&a.state[kStateTicket], 1u, PACER_AGENT);
        const int last = ticket == gridDim.x - 1u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;

    // ---- choice (the last block): ethcnn_budget_choose of this frame, the table read with agent-scope atomic loads
    const int K = a.rungs - 1;
    auto cost_of = [&](int k) -> u64 {  // (fits in 64 bits: the host checked the frame's bound)
        const unsigned* row = a.checked + (long)k * 4;
        u64 v = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) v += a.weight[d] * (u64)__hip_atomic_load(row + d, PACER_AGENT);
        return v;
    };
    const u64 full = cost_of(K);
    const u128 carry_in = (u128)load64(a.state + kStateCarry) | (u128)load64(a.state + kStateCarry + 2) << 64;
    const u128 allow = (u128)a.budget_ppm * full + carry_in;
    int fit = K, least = K;  // K: none
    u64 least_cost = ~0ull;
    for (int k = t; k < K; k += kThreads) {  // ascending k per lane: the first hit is the lane's smallest
        const u64 cst = cost_of(k);
        if (fit == K && (u128)cst * 1000000u <= allow) fit = k;
        if (least == K || cst < least_cost) least = k, least_cost = cst;
    }
    // the block-wide minimum of fit and of (cost, k): nothing about the ladder's order is assumed
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const int f2 = __shfl_xor(fit, o), l2 = __shfl_xor(least, o);
        const u64 c2 = __shfl_xor(least_cost, o);
        fit = f2 < fit ? f2 : fit;
        if (l2 < K && (least == K || c2 < least_cost || (c2 == least_cost && l2 < least))) least = l2, least_cost = c2;
    }
    if ((t & 63) == 0) s_fit[t >> 6] = fit, s_least[t >> 6] = least, s_cost[t >> 6] = least_cost;
    __syncthreads();
    if (t == 0) {
        fit = s_fit[0], least = s_least[0], least_cost = s_cost[0];
        for (int v = 1; v < kWaves; ++v) {
            fit = s_fit[v] < fit ? s_fit[v] : fit;
            if (s_least[v] < K && (least == K || s_cost[v] < least_cost || (s_cost[v] == least_cost && s_least[v] < least)))
                least = s_least[v], least_cost = s_cost[v];
        }
        const bool over = fit == K;
        const int at = over ? least : fit;
        const u64 cost = cost_of(at);
        const u128 carry = a.carry_mode && !over ? allow - (u128)cost * 1000000u : (u128)0;
        const u64 frame = load64(a.state + kStateFrame);
        store64(a.state + kStateFrame, frame + 1);
        store64(a.state + kStateCarry, (u64)carry);
        store64(a.state + kStateCarry + 2, (u64)(carry >> 64));
        ethcnn_pacer_result res;
        res.frame = (int64_t)frame;
        res.rung = at;
        res.over = over ? 1 : 0;
        res.cost = cost;
        res.full = full;
        res.carry_lo = (u64)carry;
        res.carry_hi = (u64)(carry >> 64);
        const int* th = a.thr + (long)at * 6;
#pragma unroll
        for (int l = 0; l < 3; ++l) res.up_k[l] = th[l], res.down_k[l] = th[3 + l];
#pragma unroll
        for (int l = 0; l < 6; ++l) a.state[kStateThr + l] = (unsigned)th[l];  // the one-row table of the bake (next launch)
        if (a.d_result) *a.d_result = res;
        *a.h_result = res;
    }
    __syncthreads();  // lane 0 has read the picked rung's counters: table and ticket go back to zero for the next frame
    for (int i = t; i < a.rungs * 4; i += kThreads) __hip_atomic_store(a.checked + i, 0u, PACER_AGENT);
    if (t == 0) __hip_atomic_store(&a.state[kStateTicket], 0u, PACER_AGENT);
}

__global__ void k_pacer_done(unsigned* h_done, unsigned seq) { __hip_atomic_store(h_done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
}  // namespace

long frame_blocks(long per, int rungs) {
    const long slices = (per + kSliceCtus - 1) / kSliceCtus, rung_blocks = (rungs + kThreads - 1) / kThreads;
    return slices * rung_blocks;
}

void launch_frame(hipStream_t s, const FrameArgs& a) {
    if (a.per <= 0 || a.rungs < 2) return;
    // sized for latency: slices of at most kSliceCtus CTUs, balanced, each under every rung block
    const long slices = ((long)a.per + kSliceCtus - 1) / kSliceCtus;
    const int slice_len = (int)((a.per + slices - 1) / slices);
    const int rung_blocks = (a.rungs + kThreads - 1) / kThreads;
    const long nslices = ((long)a.per + slice_len - 1) / slice_len;
    k_pacer_frame<<<(unsigned)(nslices * rung_blocks), kThreads, 0, s>>>(a, rung_blocks, slice_len);
}

void launch_done(hipStream_t s, unsigned* h_done, unsigned seq) { k_pacer_done<<<1, 1, 0, s>>>(h_done, seq); }

}  // namespace pacer
}  // namespace ethcnn
