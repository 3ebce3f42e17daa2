// ethcnn_decide.hip -- the kernel of the partition decisions (layouts and launch notes: ethcnn_decide.h; the contract: include/ethcnn.h
// "partition decisions").  The rule is the simulator's (ethcnn_sim.hip, k_sim_eval) with the roles turned round: there a lane is a
// candidate and walks the CTUs, here a lane is a CTU under the one candidate, and what k_sim_eval adds up is written out per node.
// Integers and bit masks only.
#include <hip/hip_runtime.h>

#include "ethcnn_decide.h"
#include "ethcnn_node_masks.h"
#include "ethcnn_sim.h"

namespace ethcnn {
namespace decide {

namespace {
using sim::kL1;
using sim::kL2;
using sim::raster_of;
constexpr int kThreads = 256;
constexpr int kNout = 21;
constexpr int kCodeDwords = kCodeBytes / 4;

__device__ __forceinline__ void store_block16(uint8_t* dst, long ctu, const unsigned v[4], bool wide) {
    if (wide) {
        reinterpret_cast<uint4*>(dst)[ctu] = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
        unsigned* q = reinterpret_cast<unsigned*>(dst) + ctu * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) q[r] = v[r];
    }
}

__global__ __launch_bounds__(kThreads) void k_decide(const uint4* __restrict__ recs, const unsigned* __restrict__ m, long n, Cand c, Planes pl,
                                                     unsigned* __restrict__ codes, uint8_t* __restrict__ reach, uint8_t* __restrict__ depth, int wide_reach,
                                                     int wide_depth) {
    __shared__ unsigned s_codes[kThreads * kCodeDwords];
    const int t = threadIdx.x;
    const long base = (long)blockIdx.x * kThreads;
    const int cur = (int)(n - base < kThreads ? n - base : kThreads);
    if (t < cur) {
        const long ctu = base + t;
        unsigned w[sim::kRecDwords];
        {
            const uint4* r = recs + ctu * 4;
            const uint4 a = r[0], b = r[1], e = r[2], d = r[3];
            w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
            w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
            w[8] = e.x, w[9] = e.y, w[10] = e.z, w[11] = e.w;
            w[12] = d.x, w[13] = d.y, w[14] = d.z, w[15] = d.w;
        }
        // the masks "bin > up", "bin <= down" and "bin > mid" of the 21 nodes
        unsigned so = 0u, le = 0u, gm = 0u;
#pragma unroll
        for (int k = 0; k < kNout; ++k) {
            const int bin = (int)(w[k >> 1] >> (16 * (k & 1)) & 0xffffu);
            const int l = k == 0 ? 0 : k < 5 ? 1 : 2;
            so |= (bin > c.up[l] ? 1u : 0u) << k;
            le |= (bin <= c.down[l] ? 1u : 0u) << k;
            gm |= (bin > c.mid ? 1u : 0u) << k;
        }
        const unsigned inside = w[11], edge = w[12], corner = w[13], truth = w[14];
        const bool live = ((inside | edge) & 1u) != 0u;  // a rejected CTU has empty masks
        // the gates, as k_sim_eval applies them: a closed gate zeroes the level's bins before the rule
        const int g1 = c.gate_order == 1 ? c.down[0] : c.gate_order == 2 ? c.up[0] : -2, g2 = c.gate_order == 1 ? c.down[1] : c.gate_order == 2 ? c.up[1] : -2;
        const int M1 = (int)m[2 * (size_t)w[15]], M2 = (int)m[2 * (size_t)w[15] + 1];
        const bool open1 = M1 > g1, open2 = (open1 ? M2 : 0) > g2;
        const unsigned closed = (open1 ? 0u : kL1) | (open2 ? 0u : kL2);
        const unsigned zero_le = (c.down[1] >= 0 ? kL1 : 0u) | (c.down[2] >= 0 ? kL2 : 0u);
        so &= ~closed;
        gm &= ~closed;  // (mid >= 0: a zeroed bin is never above it)
        le = (le & ~closed) | (closed & zero_le);
        const sim::Descent ds = sim::descend(so, le, inside, edge);
        const unsigned rec = ds.rec, dec = ds.dec, edg = ds.edg, d_so = ds.d_so, d_co = ds.d_co, d_bo = ds.d_bo;
        const unsigned t_split = truth & 0x1fffffu, t_unsplit = (truth >> 31 ? ~truth : 0u) & 0x1fffffu;
        const unsigned wrong = (d_so & t_unsplit) | (d_co & t_split);
        const unsigned cur_m = d_co | d_bo;           // the node itself can be the leaf
        const unsigned spl_m = d_so | d_bo | edg;     // the search goes below the node
        const unsigned pref = d_so | edg | (d_bo & gm);  // the preferred partition splits the node
        const unsigned act = dec | edg;               // visited and (partly) inside the picture
        const unsigned n8 = 4u * __popc(dec & rec & kL2) + 2u * __popc(edg & kL2) - __popc(edg & corner);
        const unsigned flags = (wrong ? 1u : 0u) | (truth >> 31) << 1 | (live ? 0u : 4u) | (live && !open1 ? 8u : 0u) | (live && !open2 ? 16u : 0u);

        // ---- codes: bit 0 = the CU is checked, bit 1 = decided and goes below, 4 = frame edge, 8 = against the label
        unsigned cw[kCodeDwords];
#pragma unroll
        for (int i = 0; i < kCodeDwords; ++i) cw[i] = 0u;
#pragma unroll
        for (int k = 0; k < kNout; ++k) {
            const int r = raster_of(k);
            const unsigned code = (cur_m >> k & 1u) | ((d_so | d_bo) >> k & 1u) << 1 | (edg >> k & 1u) << 2 | (wrong >> k & 1u) << 3;
            cw[r >> 2] |= code << (8 * (r & 3));
        }
        cw[5] |= flags << 8 | n8 << 16;
#pragma unroll
        for (int i = 0; i < kCodeDwords; ++i) s_codes[t * kCodeDwords + i] = cw[i];

        // ---- reach and the preferred depth of the 16 blocks, raster
        unsigned rw[4] = {0u, 0u, 0u, 0u}, dw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const int bx = b & 3, by = b >> 2, j = (bx >> 1) + 2 * (by >> 1), i = (bx & 1) + 2 * (by & 1);
            const int k32 = 1 + j, k16 = 5 + 4 * j + i;
            const unsigned s0 = spl_m & 1u, s1 = s0 & (spl_m >> k32), s2 = s1 & (spl_m >> k16);
            const unsigned rb = (cur_m & 1u) | (s0 & (cur_m >> k32)) << 1 | (s1 & (cur_m >> k16) & 1u) << 2 | (s2 & 1u) << 3;
            rw[by] |= (rb & 0xfu) << (8 * bx);
            unsigned dv;
            if (!live) dv = 255u;
            else if (!(pref & 1u)) dv = 0u;
            else if (!(act >> k32 & 1u)) dv = 255u;
            else if (!(pref >> k32 & 1u)) dv = 1u;
            else if (!(act >> k16 & 1u)) dv = 255u;
            else dv = 2u + (pref >> k16 & 1u);
            dw[by] |= dv << (8 * bx);
        }
        if (reach) store_block16(reach, ctu, rw, wide_reach != 0);
        if (depth) store_block16(depth, ctu, dw, wide_depth != 0);
        if (pl.p) {  // rows 4 cy + r and columns 4 cx .. of label plane f, as far as they lie in the picture
            const long per = (long)pl.ctus_w * pl.ctus_h, f = ctu / per;
            const int rem = (int)(ctu - f * per), cy = rem / pl.ctus_w, cx = rem - cy * pl.ctus_w;
            const int cols = pl.w16 - 4 * cx < 4 ? pl.w16 - 4 * cx : 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (4 * cy + r >= pl.h16) break;
                uint8_t* q = pl.p + ((f * pl.h16 + 4 * cy + r) * (long)pl.w16 + 4 * cx);
                if (cols == 4 && reinterpret_cast<uintptr_t>(q) % 4 == 0) {
                    *reinterpret_cast<unsigned*>(q) = dw[r];
                } else {
                    for (int i = 0; i < cols; ++i) q[i] = (uint8_t)(dw[r] >> (8 * i));
                }
            }
        }
    }
    if (!codes) return;  // (the same for the whole grid)
    __syncthreads();
    unsigned* dst = codes + base * kCodeDwords;
#pragma unroll
    for (int i = 0; i < kCodeDwords; ++i) {
        const int at = t + kThreads * i;
        if (at < cur * kCodeDwords) dst[at] = s_codes[at];
    }
}
}  // namespace

void launch_decide(hipStream_t s, const unsigned* recs, const unsigned* m, long n, const Cand& c, const Planes& pl, uint8_t* codes, uint8_t* reach,
                   uint8_t* depth) {
    if (n <= 0 || (!codes && !reach && !depth && !pl.p)) return;
    const long blocks = (n + kThreads - 1) / kThreads;
    k_decide<<<(unsigned)blocks, kThreads, 0, s>>>(reinterpret_cast<const uint4*>(recs), m, n, c, pl, reinterpret_cast<unsigned*>(codes), reach, depth,
                                                   reinterpret_cast<uintptr_t>(reach) % 16 == 0, reinterpret_cast<uintptr_t>(depth) % 16 == 0);
}

}  // namespace decide
}  // namespace ethcnn
