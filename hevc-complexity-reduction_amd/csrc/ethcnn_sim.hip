// ethcnn_sim.hip -- the two kernels of the partition-search simulator (record layout and launch list: ethcnn_sim.h; the rule:
// include/ethcnn.h "partition-search simulation").  Integers only: no float is accumulated anywhere, so the counters are exact and
// independent of the schedule.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ethcnn_sim.h"

namespace ethcnn {
namespace sim {

namespace {
constexpr int kThreads = 256;
constexpr int kNout = 21;

// ---------------------------------------------------------------------------------------------------------------------- pack ---
// One lane per CTU; a block stages the 21 probabilities of 256 CTUs (contiguous floats in either layout) so that the loads are
// coalesced, then each lane builds its record: bins, geometry masks, truth mask (label gather as in k_calib_count: an aligned dword
// per row where the layout allows it, four byte loads else), sub-batch index.  M1 / M2 are reduced with integer max: once per wave
// when the wave lies in one sub-batch, per lane else.
__global__ __launch_bounds__(kThreads) void k_sim_pack(const float* __restrict__ probs, const uint8_t* __restrict__ labels, long n, Geom g,
                                                       int rows_aligned, unsigned sub_base, uint4* __restrict__ recs, unsigned* __restrict__ m,
                                                       unsigned long long* __restrict__ call) {
    __shared__ float s_p[kThreads * kNout];
    const int t = threadIdx.x;
    const long ntiles = (n + kThreads - 1) / kThreads;
    const long per = (long)g.ctus_w * g.ctus_h;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long base = tile * kThreads;
        const int cur = (int)(n - base < kThreads ? n - base : kThreads);
        const float* src = probs + base * kNout;
        for (int i = t; i < cur * kNout; i += kThreads) s_p[i] = src[i];
        __syncthreads();
        const bool valid = t < cur;
        unsigned sub = 0u, m1 = 0u, m2 = 0u;
        bool whole = false, labelled = false, rejected = false, bad = false;
        if (valid) {
            int rw = 64, rh = 64, cx = 0, cy = 0;  // rw x rh: the part of the CTU inside the picture
            long f = 0;
            if (g.ctus_w) {
                const long ctu = base + t;
                f = ctu / per;
                const int rem = (int)(ctu - f * per);
                cy = rem / g.ctus_w;
                cx = rem - cy * g.ctus_w;
                rw = g.width - 64 * cx < 64 ? g.width - 64 * cx : 64;
                rh = g.height - 64 * cy < 64 ? g.height - 64 * cy : 64;
                sub = sub_base + (unsigned)(f * g.subs + rem / 1024);
            }
            whole = rw == 64 && rh == 64;
            unsigned w[kRecDwords];
#pragma unroll
            for (int i = 0; i < kRecDwords; ++i) w[i] = 0u;
            unsigned inside = 0u, edge = 0u, corner = 0u;
#pragma unroll
            for (int k = 0; k < kNout; ++k) {
                // node k: its raster index among the 21 probabilities and its square inside the CTU
                const int q = k - 5, j = k < 5 ? k - 1 : q >> 2, i = q & 3;
                const int bx = k == 0 ? 0 : k < 5 ? j & 1 : 2 * (j & 1) + (i & 1), by = k == 0 ? 0 : k < 5 ? j >> 1 : 2 * (j >> 1) + (i >> 1);
                const int s = k == 0 ? 64 : k < 5 ? 32 : 16, ox = bx * s, oy = by * s;
                const int r = k == 0 ? 0 : k < 5 ? 1 + bx + 2 * by : 5 + bx + 4 * by;
                const float p = s_p[t * kNout + r];
                const unsigned bits = __float_as_uint(p);
                if (bits > 0x3f800000u && bits != 0x80000000u) rejected = true;  // NaN, below 0, above 1 (-0 is 0)
                int bin = (int)ceilf(p * 1024.f);                                // exact product, 0..1024
                if (bin == 0 && (bits & 0x7fffffffu)) bin = 1;                   // p > 0 never lands in bin 0, whatever the denormal mode
                bin = bin < 0 ? 0 : bin > 1024 ? 1024 : bin;                     // (a rejected CTU's bins are never used)
                w[k >> 1] |= (unsigned)bin << (16 * (k & 1));
                if (k == 0) m1 = (unsigned)bin;
                if (k >= 1 && k < 5) m2 = m2 > (unsigned)bin ? m2 : (unsigned)bin;
                if (ox + s <= rw && oy + s <= rh) inside |= 1u << k;
                else if (ox < rw && oy < rh) {
                    edge |= 1u << k;
                    if (k >= 5 && rw - ox < 16 && rh - oy < 16) corner |= 1u << k;
                }
            }
            unsigned truth = 0u;
            if (labels && whole) {
                unsigned d[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (g.ctus_w == 0) {
                        d[r] = reinterpret_cast<const unsigned*>(labels)[(base + t) * 4 + r];
                    } else {  // rows 4 cy + r < h16 and columns 4 cx + 3 < w16 of label frame f
                        const uint8_t* q = labels + ((f * g.h16 + cy * 4 + r) * (long)g.w16 + cx * 4);
                        d[r] = rows_aligned ? *reinterpret_cast<const unsigned*>(q)
                                            : (unsigned)q[0] | (unsigned)q[1] << 8 | (unsigned)q[2] << 16 | (unsigned)q[3] << 24;
                    }
                }
                bad = ((d[0] | d[1] | d[2] | d[3]) & 0xfcfcfcfcu) != 0u;  // a depth above 3: the whole call will add nothing
                unsigned total = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    unsigned sum = 0u;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int bx = 2 * (j & 1) + (i & 1), by = 2 * (j >> 1) + (i >> 1);
                        const unsigned v = d[by] >> (8 * bx) & 0xffu;
                        sum += v;
                        if (v == 3u) truth |= 1u << (5 + 4 * j + i);
                    }
                    if (sum > 6u) truth |= 1u << (1 + j);
                    total += sum;
                }
                if (total > 8u) truth |= 1u;
                labelled = !rejected;
                truth = labelled ? truth | 0x80000000u : 0u;
            }
            if (rejected) inside = edge = corner = 0u;
            w[11] = inside;
            w[12] = edge;
            w[13] = corner;
            w[14] = truth;
            w[15] = sub;
            uint4* dst = recs + (base + t) * 4;
            dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
            dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
            dst[2] = make_uint4(w[8], w[9], w[10], w[11]);
            dst[3] = make_uint4(w[12], w[13], w[14], w[15]);
        }
        if (g.ctus_w) {
            if (!valid || rejected) m1 = m2 = 0u;
            const unsigned sub0 = __shfl(sub, 0);  // (lane 0 is valid whenever any lane of the wave is)
            if (__all(!valid || sub == sub0)) {
#pragma unroll
                for (int o = 32; o; o >>= 1) {
                    const unsigned a = __shfl_xor(m1, o), b = __shfl_xor(m2, o);
                    m1 = m1 > a ? m1 : a;
                    m2 = m2 > b ? m2 : b;
                }
                if ((t & 63) == 0) {
                    if (m1) atomicMax(&m[2 * (size_t)sub0], m1);
                    if (m2) atomicMax(&m[2 * (size_t)sub0 + 1], m2);
                }
            } else {
                if (m1) atomicMax(&m[2 * (size_t)sub], m1);
                if (m2) atomicMax(&m[2 * (size_t)sub + 1], m2);
            }
        }
        const unsigned long long nb = __popcll(__ballot(bad)), nw = __popcll(__ballot(whole && !rejected)), nl = __popcll(__ballot(labelled)),
                                 nr = __popcll(__ballot(rejected));
        if ((t & 63) == 0) {
            if (nb) atomicAdd(&call[kCallFlag], nb);
            if (nw) atomicAdd(&call[kCallWhole], nw);
            if (nl) atomicAdd(&call[kCallLabelled], nl);
            if (nr) atomicAdd(&call[kCallRejected], nr);
        }
        __syncthreads();  // the next trip overwrites the staging
    }
}

// ---------------------------------------------------------------------------------------------------------------------- eval ---
// Lane = candidate.  A wave owns 64 candidates and a slice of the CTUs; its six thresholds and 21 counters live in registers.  The
// record address is the same for the whole wave (the wave index goes through readfirstlane), so the record arrives by uniform loads
// and everything that depends on the record alone -- unpacking the bins, the truth masks -- is scalar work.  Per lane: 42 compares
// build the masks "bin > up" and "bin <= down" of the 21 nodes; the descent of the quadtree, the outcome of every node and every
// counter are then mask arithmetic and population counts, without a branch.  Nothing is reduced across lanes; a lane adds its 32-bit
// counters to its candidate's uint64 words at the end of its slice (a slice is at most kMaxSlice CTUs: 64 counts a CTU at most).
__global__ __launch_bounds__(kThreads) void k_sim_eval(const unsigned* __restrict__ recs, const unsigned* __restrict__ m, long n,
                                                       const int* __restrict__ cand, long ncand, int cand_waves, long slices, long slice_len,
                                                       int gate_order, unsigned long long* __restrict__ out) {
    const long wave = blockIdx.x * (long)(kThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long slice = wave / cand_waves;
    if (slice >= slices) return;
    const long c = (wave - slice * cand_waves) * 64 + (threadIdx.x & 63);
    const bool live = c < ncand;
    const int* th = cand + (live ? c : ncand - 1) * 6;
    const int up0 = th[0], up1 = th[1], up2 = th[2], down0 = th[3], down1 = th[4], down2 = th[5];
    // (gate thresholds of -2 keep every gate open: M >= 0)
    const int g1 = gate_order == 1 ? down0 : gate_order == 2 ? up0 : -2, g2 = gate_order == 1 ? down1 : gate_order == 2 ? up1 : -2;
    const unsigned zero_le = (down1 >= 0 ? kL1 : 0u) | (down2 >= 0 ? kL2 : 0u);  // "bin <= down" of a bin that a gate zeroed
    unsigned n_so[3] = {0u, 0u, 0u}, n_co[3] = {0u, 0u, 0u}, n_bo[3] = {0u, 0u, 0u}, n_edge[3] = {0u, 0u, 0u}, n_ws[3] = {0u, 0u, 0u},
             n_wt[3] = {0u, 0u, 0u};
    unsigned n_bad = 0u, n_rec16 = 0u, n_corner = 0u;
    const long first = slice * slice_len, last = first + slice_len < n ? first + slice_len : n;
    for (long i = first; i < last; ++i) {
        const unsigned* r = recs + i * kRecDwords;
        unsigned w[kRecDwords];
#pragma unroll
        for (int k = 0; k < kRecDwords; ++k) w[k] = r[k];
        unsigned so = 0u, le = 0u;
#pragma unroll
        for (int k = 0; k < kNout; ++k) {
            const int bin = (int)(w[k >> 1] >> (16 * (k & 1)) & 0xffffu);
            const int up = k == 0 ? up0 : k < 5 ? up1 : up2, down = k == 0 ? down0 : k < 5 ? down1 : down2;
            so |= (bin > up ? 1u : 0u) << k;
            le |= (bin <= down ? 1u : 0u) << k;
        }
        const unsigned inside = w[11], edge = w[12], corner = w[13], truth = w[14];
        const int M1 = (int)m[2 * (size_t)w[15]], M2 = (int)m[2 * (size_t)w[15] + 1];
        const bool open1 = M1 > g1, open2 = (open1 ? M2 : 0) > g2;
        const unsigned closed = (open1 ? 0u : kL1) | (open2 ? 0u : kL2);
        so &= ~closed;
        le = (le & ~closed) | (closed & zero_le);
        const unsigned co = le & ~so;
        const unsigned rec = (inside & ~co) | edge;  // a visited node with this bit visits its sub-CUs
        unsigned vis = 1u | ((0u - (rec & 1u)) & kL1);
        const unsigned t = (rec & vis) >> 1 & 0xfu, x = (t | t << 3 | t << 6 | t << 9) & 0x1111u;
        vis |= (x * 15u) << 5;
        const unsigned dec = vis & inside, edg = vis & edge;
        const unsigned d_so = dec & so, d_co = dec & co, d_bo = dec & ~so & ~le;
        const unsigned t_split = truth & 0x1fffffu, t_unsplit = (truth >> 31 ? ~truth : 0u) & 0x1fffffu;
        const unsigned w_so = d_so & t_unsplit, w_co = d_co & t_split;
        n_so[0] += d_so & 1u;
        n_so[1] += __popc(d_so & kL1);
        n_so[2] += __popc(d_so & kL2);
        n_co[0] += d_co & 1u;
        n_co[1] += __popc(d_co & kL1);
        n_co[2] += __popc(d_co & kL2);
        n_bo[0] += d_bo & 1u;
        n_bo[1] += __popc(d_bo & kL1);
        n_bo[2] += __popc(d_bo & kL2);
        n_edge[0] += edg & 1u;
        n_edge[1] += __popc(edg & kL1);
        n_edge[2] += __popc(edg & kL2);
        n_ws[0] += w_so & 1u;
        n_ws[1] += __popc(w_so & kL1);
        n_ws[2] += __popc(w_so & kL2);
        n_wt[0] += w_co & 1u;
        n_wt[1] += __popc(w_co & kL1);
        n_wt[2] += __popc(w_co & kL2);
        n_bad += (w_so | w_co) ? 1u : 0u;
        n_rec16 += __popc(dec & rec & kL2);
        n_corner += __popc(edg & corner);
    }
    if (!live) return;
    unsigned long long* o = out + c * kFields;
    auto add = [&](int field, unsigned long long v) {
        if (v) atomicAdd(&o[field], v);
    };
    // the field order of ethcnn_sim_counts; 8 x 8 CUs: four under a recursing 16 x 16 node, two (one in the corner) under an edge node
    for (int d = 0; d < 3; ++d) add(d, (unsigned long long)n_co[d] + n_bo[d]);
    add(3, 4ull * n_rec16 + 2ull * n_edge[2] - n_corner);
    for (int d = 0; d < 3; ++d) {
        add(4 + d, n_so[d]);
        add(7 + d, n_co[d]);
        add(10 + d, n_bo[d]);
        add(13 + d, n_edge[d]);
        add(16 + d, n_ws[d]);
        add(19 + d, n_wt[d]);
    }
    add(22, n_bad);
}
}  // namespace

void launch_pack(hipStream_t s, const float* probs, const uint8_t* labels, long n, const Geom& g, unsigned sub_base, unsigned* recs, unsigned* m,
                 unsigned long long* call, int cus) {
    if (n <= 0) return;
    const long ntiles = (n + kThreads - 1) / kThreads;
    const int grid = (int)(ntiles < 8L * cus ? ntiles : 8L * cus);
    const int rows_aligned = g.ctus_w != 0 && g.w16 % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % 4 == 0;
    k_sim_pack<<<grid, kThreads, 0, s>>>(probs, labels, n, g, rows_aligned, sub_base, reinterpret_cast<uint4*>(recs), m, call);
}

void launch_eval(hipStream_t s, const unsigned* recs, const unsigned* m, long n, const int* cand, long ncand, int gate_order, unsigned long long* out,
                 int cus) {
    if (n <= 0 || ncand <= 0) return;
    // waves = candidate groups x slices: about 16 waves a CU, slices of at least 64 and at most kMaxSlice CTUs
    const long cand_waves = (ncand + 63) / 64;
    long slices = (16L * cus + cand_waves - 1) / cand_waves;
    slices = std::min(slices, (n + 63) / 64);
    slices = std::max(std::max(slices, 1L), (n + kMaxSlice - 1) / kMaxSlice);
    const long slice_len = (n + slices - 1) / slices;
    slices = (n + slice_len - 1) / slice_len;
    const long blocks = (cand_waves * slices + kThreads / 64 - 1) / (kThreads / 64);
    k_sim_eval<<<(unsigned)blocks, kThreads, 0, s>>>(recs, m, n, cand, ncand, (int)cand_waves, slices, slice_len, gate_order, out);
}

}  // namespace sim
}  // namespace ethcnn
