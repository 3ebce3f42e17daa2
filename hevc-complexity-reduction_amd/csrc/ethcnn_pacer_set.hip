// ethcnn_pacer_set.hip -- the two kernels of the pacer set (layouts and launch notes: ethcnn_pacer_set.h; the contract: include/ethcnn.h
// "search budget, online: several sequences").  k_pacer_table is k_pacer_frame (ethcnn_pacer.hip) over a table of frames, each with the
// table, the ticket, the carry and the result slot of its own SLOT; k_pacer_bake_table is k_budget_bake (ethcnn_budget.hip) over the same
// table, each frame under the row its slot's choice left behind.  The rule on a record is shared with k_decide, k_budget_* and
// k_pacer_frame through ethcnn_node_masks.h.  Integers and bit masks only.  Ladder, weights, budget and mode are those of the POLICY the
// segment's slot is bound to (ethcnn_pacer_set.h "POLICIES"): k_pacer_table<true> reads its record from the policy table in HBM,
// k_pacer_table<false>, for a set of one policy, from the kernel argument.
//
// The packing arithmetic, the 64-bit state accessors and the bake arithmetic are RESTATED here rather than shared through a header with
// ethcnn_pacer.hip and ethcnn_budget.hip: those two files compile to what they compiled to before this one existed.
#include <hip/hip_runtime.h>

#include "ethcnn_spec.h"
#include "ethcnn_node_masks.h"
#include "ethcnn_pacer_set.h"
#include "ethcnn_sim.h"

namespace ethcnn {
namespace pacer {

namespace {
using sim::kL1;
using sim::kL2;
using sim::kRecDwords;
constexpr int kThreads = kPacerSetThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kNout = 21;
constexpr unsigned kOne = 0x3f800000u, kHalf = 0x3f000000u;  // 1.0f, 0.5f (0.0f is 0)
typedef unsigned __int128 u128;
typedef unsigned long long u64;
static_assert(kSliceCtus == kPacerSetSliceCtus, "the plan cuts the slices the kernel holds in LDS");

#define PACER_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// one CTU: 21 probabilities in raster order -> its record (truth = 0, sub-batch = 0); rw x rh is the part of the CTU inside the picture
// (k_pacer_frame's pack_ctu, which restates k_sim_pack's)
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

// kMany: the set holds several policies and the segment's record is read from the policy table in HBM; otherwise the set's one policy
// stands in the kernel argument, as ladder, weights, budget and mode did before there were policies, and the block loads nothing for it
template <bool kMany>
__global__ __launch_bounds__(kThreads) void k_pacer_table(const FrameTable tb) {
    __shared__ uint4 s_rec[kSliceCtus * 4];
    __shared__ float s_p[kSliceCtus * kNout];
    __shared__ u64 s_cost[kWaves];
    __shared__ int s_fit[kWaves], s_least[kWaves];
    __shared__ int s_last;
    const int t = threadIdx.x;
    // ---- the block's segment: a scalar walk (the block index is uniform; first_block rises along the table)
    const int B = (int)blockIdx.x;
    int j = 0;
    for (int i = 1; i < tb.nseg; ++i)
        if (tb.seg[i].first_block <= B) j = i;
    const TableSeg sg = tb.seg[j];
    // ---- the segment's policy: one record, read once (its index is block-uniform like the segment: scalar loads)
    const PolicyRec pr = kMany ? tb.policy[sg.policy] : tb.one;
    const int rungs = pr.rungs, rung_blocks = sg.rung_blocks;
    const int* const thr = kMany ? tb.thr + (long)pr.first_row * 6 : tb.thr;  // its ladder: rows 0 .. rungs - 1 and no other
    unsigned* const checked = tb.checked + (long)sg.slot * tb.stride * 4;  // the slot's table, state words and result slot
    unsigned* const state = tb.state + sg.slot * kStateWords;
    const int local = B - sg.first_block;                              // 0 .. nblocks - 1 of the segment
    const int slice = local / rung_blocks, rb = local - slice * rung_blocks;
    const int first = slice * sg.slice_len;
    const int cur = sg.per - first < sg.slice_len ? sg.per - first : sg.slice_len;  // 1..kSliceCtus

    // ---- pack: the slice's probabilities through LDS (coalesced), a lane per CTU
    {
        const float* src = sg.probs + (long)first * kNout;
        for (int i = t; i < cur * kNout; i += kThreads) s_p[i] = src[i];
    }
    __syncthreads();
    if (t < cur) {
        const int ctu = first + t, cy = ctu / sg.ctus_w, cx = ctu - cy * sg.ctus_w;
        const int rw = sg.width - 64 * cx < 64 ? sg.width - 64 * cx : 64, rh = sg.height - 64 * cy < 64 ? sg.height - 64 * cy : 64;
        unsigned w[kRecDwords];
        pack_ctu(s_p + t * kNout, rw, rh, w);
        s_rec[t * 4 + 0] = make_uint4(w[0], w[1], w[2], w[3]);
        s_rec[t * 4 + 1] = make_uint4(w[4], w[5], w[6], w[7]);
        s_rec[t * 4 + 2] = make_uint4(w[8], w[9], w[10], w[11]);
        s_rec[t * 4 + 3] = make_uint4(w[12], w[13], w[14], w[15]);
    }
    __syncthreads();
    if (rb == 0) {  // one rung group of the slice keeps the records for the bake
        uint4* dst = reinterpret_cast<uint4*>(tb.recs) + (sg.rec0 + first) * 4;
        if (t < cur * 4) dst[t] = s_rec[t];
    }

    // ---- count: a lane is a rung, the wave walks the slice's records (every lane reads the same LDS address)
    {
        const int c = (rb * kWaves + (t >> 6)) * 64 + (t & 63);
        const bool live = c < rungs;
        const int* th = thr + (long)(live ? c : rungs - 1) * 6;  // a dead lane reads its OWN policy's last row, counts nothing
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
            unsigned* o = checked + (long)c * 4;
            if (n64) __hip_atomic_fetch_add(&o[0], n64, PACER_AGENT);
            if (n32) __hip_atomic_fetch_add(&o[1], n32, PACER_AGENT);
            if (n16) __hip_atomic_fetch_add(&o[2], n16, PACER_AGENT);
            if (n8) __hip_atomic_fetch_add(&o[3], n8, PACER_AGENT);
        }
    }

    // ---- ticket of the SEGMENT: every wave's adds and stores are performed, then one lane releases and draws; nobody waits for anybody
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(&state[kStateTicket], 1u, PACER_AGENT);
        const int last = ticket == (unsigned)sg.nblocks - 1u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;

    // ---- choice (the segment's last block): ethcnn_budget_choose of this frame, the slot's table read with agent-scope atomic loads
    const int K = rungs - 1;
    auto cost_of = [&](int k) -> u64 {  // (fits in 64 bits: the host checked the frame's bound)
        const unsigned* row = checked + (long)k * 4;
        u64 v = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) v += pr.weight[d] * (u64)__hip_atomic_load(row + d, PACER_AGENT);
        return v;
    };
    const u64 full = cost_of(K);
    const u128 carry_in = (u128)load64(state + kStateCarry) | (u128)load64(state + kStateCarry + 2) << 64;
    const u128 allow = (u128)pr.budget_ppm * full + carry_in;
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
        const u128 carry = pr.carry_mode && !over ? allow - (u128)cost * 1000000u : (u128)0;
        const u64 frame = load64(state + kStateFrame);
        store64(state + kStateFrame, frame + 1);
        store64(state + kStateCarry, (u64)carry);
        store64(state + kStateCarry + 2, (u64)(carry >> 64));
        ethcnn_pacer_result res;
        res.frame = (int64_t)frame;
        res.rung = at;
        res.over = over ? 1 : 0;
        res.cost = cost;
        res.full = full;
        res.carry_lo = (u64)carry;
        res.carry_hi = (u64)(carry >> 64);
        const int* th = thr + (long)at * 6;
#pragma unroll
        for (int l = 0; l < 3; ++l) res.up_k[l] = th[l], res.down_k[l] = th[3 + l];
#pragma unroll
        for (int l = 0; l < 6; ++l) state[kStateThr + l] = (unsigned)th[l];  // the slot's one-row table of the bake (next launch)
        if (sg.d_result) *sg.d_result = res;
        tb.h_result[sg.slot] = res;
    }
    __syncthreads();  // lane 0 has read the picked rung's counters: the slot's table and ticket go back to zero for its next frame
    for (int i = t; i < rungs * 4; i += kThreads) __hip_atomic_store(checked + i, 0u, PACER_AGENT);
    if (t == 0) __hip_atomic_store(&state[kStateTicket], 0u, PACER_AGENT);
}

__global__ __launch_bounds__(kThreads) void k_pacer_bake_table(const BakeTable tb) {
    __shared__ unsigned s_rows[kThreads * kNout];
    const int t = threadIdx.x;
    const int B = (int)blockIdx.x;
    int j = 0;
    for (int i = 1; i < tb.nseg; ++i)
        if (tb.seg[i].first_block <= B) j = i;
    const BakeSeg sg = tb.seg[j];
    const int base = (B - sg.first_block) * kThreads;  // the block's first CTU in its frame
    const int cur = sg.per - base < kThreads ? sg.per - base : kThreads;
    if (t < cur) {
        unsigned w[kRecDwords];
        {
            const uint4* r = reinterpret_cast<const uint4*>(tb.recs) + (sg.rec0 + base + t) * 4;
            const uint4 a = r[0], b = r[1], e = r[2], d = r[3];
            w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
            w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
            w[8] = e.x, w[9] = e.y, w[10] = e.z, w[11] = e.w;
            w[12] = d.x, w[13] = d.y, w[14] = d.z, w[15] = d.w;
        }
        const int* th = reinterpret_cast<const int*>(tb.state + sg.slot * kStateWords + kStateThr);
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
    unsigned* dst = sg.baked + (long)base * kNout;
#pragma unroll
    for (int i = 0; i < kNout; ++i) {
        const int at = t + kThreads * i;
        if (at < cur * kNout) dst[at] = s_rows[at];
    }
}
}  // namespace

void launch_table(hipStream_t s, const FrameTable& t, unsigned blocks, bool many) {
    if (many) k_pacer_table<true><<<blocks, kThreads, 0, s>>>(t);
    else k_pacer_table<false><<<blocks, kThreads, 0, s>>>(t);
}

void launch_bake_table(hipStream_t s, const BakeTable& t, unsigned blocks) { k_pacer_bake_table<<<blocks, kThreads, 0, s>>>(t); }

}  // namespace pacer
}  // namespace ethcnn
