// ethcnn_node_masks.h -- the rule of include/ethcnn.h "partition-search simulation" on one CTU record (ethcnn_sim.h) as bit masks over its
// 21 nodes in QUAD order, shared by the kernels that hold one record and one candidate per lane or per wave: k_decide
// (ethcnn_decide.hip: the descent; its compare loop also builds the "bin > mid" mask and stays there), k_budget_cost and k_budget_bake
// (ethcnn_budget.hip), k_reach_hist (ethcnn_reach.hip: the descent and the batch gates).  Integers only.
#pragma once
#include <hip/hip_runtime.h>

#include "ethcnn_sim.h"

namespace ethcnn {
namespace sim {

// quad-order node k -> its raster index among the 21 probabilities (ethcnn_sim.hip, k_sim_pack)
__host__ __device__ constexpr int raster_of(int k) {
    return k < 5 ? k : 5 + (2 * (((k - 5) >> 2) & 1) + ((k - 5) & 1)) + 4 * (2 * (((k - 5) >> 2) >> 1) + (((k - 5) & 3) >> 1));
}

// the masks "bin > up" and "bin <= down" of the 21 nodes of record w under one candidate (up / down per level)
__device__ __forceinline__ void compare_bins(const unsigned* w, const int* up, const int* down, unsigned& so, unsigned& le) {
    so = le = 0u;
#pragma unroll
    for (int k = 0; k < 21; ++k) {
        const int bin = (int)(w[k >> 1] >> (16 * (k & 1)) & 0xffffu);
        const int l = k == 0 ? 0 : k < 5 ? 1 : 2;
        so |= (bin > up[l] ? 1u : 0u) << k;
        le |= (bin <= down[l] ? 1u : 0u) << k;
    }
}

// the batch gates (include/ethcnn.h "partition-search simulation", Gates) as k_sim_eval applies them: the gate thresholds of a candidate
// under gate_order (-2 keeps every gate open: M >= 0) ...
__device__ __forceinline__ void gate_thresholds(int gate_order, const int* up, const int* down, int& g1, int& g2) {
    g1 = gate_order == 1 ? down[0] : gate_order == 2 ? up[0] : -2;
    g2 = gate_order == 1 ? down[1] : gate_order == 2 ? up[1] : -2;
}

// ... and the levels whose bins the closed gates of sub-batch `sub` zero (kL1, kL2 or both), with so / le corrected to what a bin of 0
// gives: never "bin > up", and "bin <= down" exactly when down >= 0.  m: M1 / M2 per sub-batch (sub-batch 0 = none: kNoGate, never closed)
__device__ __forceinline__ unsigned close_gates(const unsigned* __restrict__ m, unsigned sub, int g1, int g2, const int* down, unsigned& so, unsigned& le) {
    const int M1 = (int)m[2 * (size_t)sub], M2 = (int)m[2 * (size_t)sub + 1];
    const bool open1 = M1 > g1, open2 = (open1 ? M2 : 0) > g2;
    const unsigned closed = (open1 ? 0u : kL1) | (open2 ? 0u : kL2);
    const unsigned zero_le = (down[1] >= 0 ? kL1 : 0u) | (down[2] >= 0 ? kL2 : 0u);
    so &= ~closed;
    le = (le & ~closed) | (closed & zero_le);
    return closed;
}

// the descent of the quadtree: which nodes are visited and how each decided node comes out
struct Descent {
    unsigned co;   // "bin <= down" and not "bin > up": HM tests "split only" first
    unsigned rec;  // a visited node with this bit visits its sub-CUs
    unsigned dec;  // visited and wholly inside the picture: a decided node
    unsigned edg;  // visited and across the frame edge (rule 3)
    unsigned d_so, d_co, d_bo;  // the decided nodes by outcome: SPLIT ONLY, CURRENT ONLY, BOTH
};

__device__ __forceinline__ Descent descend(unsigned so, unsigned le, unsigned inside, unsigned edge) {
    Descent d;
    d.co = le & ~so;
    d.rec = (inside & ~d.co) | edge;
    unsigned vis = 1u | ((0u - (d.rec & 1u)) & kL1);
    const unsigned tt = (d.rec & vis) >> 1 & 0xfu, x = (tt | tt << 3 | tt << 6 | tt << 9) & 0x1111u;
    vis |= (x * 15u) << 5;
    d.dec = vis & inside;
    d.edg = vis & edge;
    d.d_so = d.dec & so;
    d.d_co = d.dec & d.co;
    d.d_bo = d.dec & ~so & ~le;
    return d;
}

}  // namespace sim
}  // namespace ethcnn
