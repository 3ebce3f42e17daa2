// ethcnn_ladder_step.h -- one step of the greedy ladder walk as a device function, shared by the two kernels that take it:
// k_ladder_step (ethcnn_ladder.hip: a move is weighed by the newly bad CTUs, which needs labels) and k_ladder_step_risk
// (ethcnn_risk.hip: by the expected wrong decisions, which does not).  The launch shape, the state block, the ticket and the rule of
// the choice are described in ethcnn_ladder.h; the rule itself in include/ethcnn.h "search budget: building a ladder".  What the two
// differ in comes from a kind K:
//   K::Args         the launch arguments: recs, n, state, table, rungs, weight[4], grid, slots, values, max_rungs and the kind's own
//   K::Rung         the rung record appended to a.rungs; it starts with thr, coord, value, checked[4]
//   K::kFields      uint64 words of a table row: checked[0..3], then the kind's own
//   K::Count        a lane's own counters: record(a, w, ds) per CTU record, flush(o) into the lane's table row after its slice
//   K::harm(row)    what the choice weighs against the saving (read with agent-scope atomic loads); the state word kStateBad holds
//                   that of the current rung
//   K::over_cap(a, harm)   rule 4: the coordinate has no move
//   K::finish(rung, row)   the kind's own fields of the appended rung
// Integers and bit masks only.
#pragma once
#include <hip/hip_runtime.h>

#include "ethcnn_ladder.h"
#include "ethcnn_node_masks.h"
#include "ethcnn_sim.h"

namespace ethcnn {
namespace ladder {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kNone = 0x7fffffff;
typedef unsigned __int128 u128;
typedef __int128 i128;
typedef unsigned long long u64;

#define LADDER_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// the values a coordinate may move to: a down in (down_k, up_k], an up in [max(down_k, 0), up_k) -- so down_k <= up_k on every rung
__device__ __forceinline__ bool in_range(int c, int v, const int* up, const int* down) {
    const int d = c >> 1;
    const int u = d == 0 ? up[0] : d == 1 ? up[1] : up[2], dn = d == 0 ? down[0] : d == 1 ? down[1] : down[2];
    return c & 1 ? v >= (dn > 0 ? dn : 0) && v < u : v > dn && v <= u;
}

template <class K>
__device__ __forceinline__ void step(const unsigned* __restrict__ recs, const typename K::Args& a, const int coord_waves, const long slices,
                                     const long slice_len) {
    using sim::kL1;
    using sim::kL2;
    using sim::kRecDwords;
    __shared__ int s_best[kWaves][6];
    __shared__ int s_last;
    const int t = threadIdx.x;
    // the flag changes only in a launch's last block, behind every ticket: the whole grid reads the same value
    if (__hip_atomic_load(&a.state[kStateDone], LADDER_AGENT)) return;
    int up[3], down[3];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        up[l] = (int)(long long)__hip_atomic_load(&a.state[kStateUp + l], LADDER_AGENT);
        down[l] = (int)(long long)__hip_atomic_load(&a.state[kStateDown + l], LADDER_AGENT);
        up[l] = __builtin_amdgcn_readfirstlane(up[l]);  // the same in every lane: what does not depend on the lane's value is scalar work
        down[l] = __builtin_amdgcn_readfirstlane(down[l]);
    }

    // ---- count: a lane is a candidate, the wave walks its slice of the records (one address for the whole wave)
    {
        const long wave = blockIdx.x * (long)kWaves + __builtin_amdgcn_readfirstlane(t >> 6);
        const int cand_waves = 6 * coord_waves;
        const long slice = wave / cand_waves;
        const int cw = (int)(wave - slice * cand_waves);
        const int c = cw / coord_waves, m = (cw - c * coord_waves) * 64 + (t & 63);
        const int v = m * a.grid;
        const bool live = slice < slices && m < a.values && in_range(c, v, up, down);
        if (__any(live)) {
            int cu[3], cd[3];
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                cu[l] = c == 2 * l + 1 ? v : up[l];
                cd[l] = c == 2 * l ? v : down[l];
            }
            unsigned n64 = 0u, n32 = 0u, n16 = 0u, n8 = 0u;
            typename K::Count own;
            const long first = slice * slice_len, last = first + slice_len < a.n ? first + slice_len : a.n;
            for (long i = first; i < last; ++i) {
                const unsigned* r = recs + i * kRecDwords;
                unsigned w[15];
#pragma unroll
                for (int k = 0; k < 15; ++k) w[k] = r[k];
                unsigned so, le;
                sim::compare_bins(w, cu, cd, so, le);
                const sim::Descent ds = sim::descend(so, le, w[11], w[12]);
                const unsigned chk = ds.dec & ~so;  // CURRENT ONLY or BOTH: the CU itself is checked
                n64 += chk & 1u;
                n32 += __popc(chk & kL1);
                n16 += __popc(chk & kL2);
                // 8 x 8 CUs: four under a recursing 16 x 16 node, two (one in the corner) under an edge node
                n8 += 4u * __popc(ds.dec & ds.rec & kL2) + 2u * __popc(ds.edg & kL2) - __popc(ds.edg & w[13]);
                own.record(a, w, ds);
            }
            if (live) {
                u64* o = a.table + ((long)c * a.slots + m) * K::kFields;
                if (n64) __hip_atomic_fetch_add(&o[0], (u64)n64, LADDER_AGENT);
                if (n32) __hip_atomic_fetch_add(&o[1], (u64)n32, LADDER_AGENT);
                if (n16) __hip_atomic_fetch_add(&o[2], (u64)n16, LADDER_AGENT);
                if (n8) __hip_atomic_fetch_add(&o[3], (u64)n8, LADDER_AGENT);
                own.flush(o);
            }
        }
    }

    // ---- ticket: every wave's adds are performed, then one lane releases and draws; nobody waits for anybody
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const u64 ticket = __hip_atomic_fetch_add(&a.state[kStateTicket], 1ull, LADDER_AGENT);
        const int last = ticket == (u64)gridDim.x - 1ull;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;

    // ---- choice (the last block): the table read with agent-scope atomic loads
    auto cost_of = [&](const u64* row) -> u64 {  // (fits in 64 bits: the host checked the set's bound)
        u64 x = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) x += a.weight[d] * __hip_atomic_load(row + d, LADDER_AGENT);
        return x;
    };
    const u64 C = __hip_atomic_load(&a.state[kStateCost], LADDER_AGENT), B = __hip_atomic_load(&a.state[kStateBad], LADDER_AGENT);
    // per coordinate the value nearest to the current one whose cost is below C: the smallest m of a down, the largest of an up
    int best[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        best[c] = kNone;
        for (int m = t; m < a.values; m += kThreads) {
            if (!in_range(c, m * a.grid, up, down)) continue;
            if (cost_of(a.table + ((long)c * a.slots + m) * K::kFields) < C) {
                const int key = c & 1 ? a.values - 1 - m : m;
                best[c] = key < best[c] ? key : best[c];
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const int b2 = __shfl_xor(best[c], o);
            best[c] = b2 < best[c] ? b2 : best[c];
        }
        if ((t & 63) == 0) s_best[t >> 6][c] = best[c];
    }
    __syncthreads();
    if (t == 0) {
        int pick = -1, pick_v = 0;
        u64 pick_den = 0, pick_cost = 0, pick_bad = 0;
        const u64* pick_row = nullptr;
        i128 pick_num = 0;
        for (int c = 0; c < 6; ++c) {
            int key = s_best[0][c];
            for (int v = 1; v < kWaves; ++v) key = s_best[v][c] < key ? s_best[v][c] : key;
            if (key == kNone) continue;  // no value of this coordinate lowers the cost
            const int m = c & 1 ? a.values - 1 - key : key;
            const u64* row = a.table + ((long)c * a.slots + m) * K::kFields;
            const u64 cost = cost_of(row), bad = K::harm(row);
            if (K::over_cap(a, bad)) continue;  // above the cap: the coordinate has no move, nothing further is looked at
            // the smallest (bad - B) / (C - cost), exactly; then the larger saving; then the smaller c
            const i128 num = (i128)bad - (i128)B;
            const u64 den = C - cost;
            bool take = pick < 0;
            if (!take) {
                const i128 lhs = num * (i128)pick_den, rhs = pick_num * (i128)den;
                take = lhs < rhs || (lhs == rhs && den > pick_den);
            }
            if (take) pick = c, pick_v = m * a.grid, pick_num = num, pick_den = den, pick_cost = cost, pick_bad = bad, pick_row = row;
        }
        const u64 nr = __hip_atomic_load(&a.state[kStateRungs], LADDER_AGENT);
        if (pick < 0 || nr >= (u64)a.max_rungs) {
            __hip_atomic_store(&a.state[kStateDone], 1ull, LADDER_AGENT);
        } else {
            typename K::Rung rung;
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                rung.thr.up_k[l] = pick == 2 * l + 1 ? pick_v : up[l];
                rung.thr.down_k[l] = pick == 2 * l ? pick_v : down[l];
            }
            rung.coord = pick;
            rung.value = pick_v;
#pragma unroll
            for (int d = 0; d < 4; ++d) rung.checked[d] = __hip_atomic_load(pick_row + d, LADDER_AGENT);
            K::finish(rung, pick_row);
            a.rungs[nr] = rung;
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                __hip_atomic_store(&a.state[kStateUp + l], (u64)(long long)rung.thr.up_k[l], LADDER_AGENT);
                __hip_atomic_store(&a.state[kStateDown + l], (u64)(long long)rung.thr.down_k[l], LADDER_AGENT);
            }
            __hip_atomic_store(&a.state[kStateCost], pick_cost, LADDER_AGENT);
            __hip_atomic_store(&a.state[kStateBad], pick_bad, LADDER_AGENT);
            __hip_atomic_store(&a.state[kStateRungs], nr + 1, LADDER_AGENT);
            if (nr + 1 >= (u64)a.max_rungs) __hip_atomic_store(&a.state[kStateDone], 1ull, LADDER_AGENT);
        }
    }
    __syncthreads();  // lane 0 has read the picked row: table and ticket go back to zero for the next step
    for (long i = t; i < 6L * a.slots * K::kFields; i += kThreads) __hip_atomic_store(a.table + i, 0ull, LADDER_AGENT);
    if (t == 0) __hip_atomic_store(&a.state[kStateTicket], 0ull, LADDER_AGENT);
}

// the sizing both kernels share: waves = candidate waves x slices, about 16 waves a CU, slices of at least 64 and at most
// sim::kMaxSlice CTUs (k_sim_eval's sizing) -> blocks
inline long step_shape(long n, int values, int cus, int* coord_waves, long* slices, long* slice_len) {
    *coord_waves = (values + 63) / 64;
    const long cand_waves = 6L * *coord_waves;
    long s = (16L * cus + cand_waves - 1) / cand_waves;
    s = s < (n + 63) / 64 ? s : (n + 63) / 64;
    s = s > 1L ? s : 1L;
    s = s > (n + sim::kMaxSlice - 1) / sim::kMaxSlice ? s : (n + sim::kMaxSlice - 1) / sim::kMaxSlice;
    *slice_len = (n + s - 1) / s;
    *slices = (n + *slice_len - 1) / *slice_len;
    return (cand_waves * *slices + kWaves - 1) / kWaves;
}

}  // namespace ladder
}  // namespace ethcnn
