// ethcnn_audit.hip -- the comparison kernel (state layout and launch rule: ethcnn_audit.h; definitions: include/ethcnn.h "comparing two
// predictions").  Integers and fp32 compares only: the one float operation is the subtraction a - b, whose bits are then handled as an
// integer, so every word of the result is exact and independent of the schedule.
#include <hip/hip_runtime.h>

#include "ethcnn_audit.h"

namespace ethcnn {
namespace audit {

namespace {
constexpr int kThreads = 256;
constexpr int kNout = 21;
constexpr unsigned kL1 = 0x1eu, kL2 = 0x1fffe0u, kAll = 0x1fffffu;  // the nodes of a level, in the node order of ethcnn_sim.h
static_assert(kTile == kThreads, "one lane per CTU of a tile");
static_assert((kTile * kNout * 4) % 16 == 0, "a tile starts 16-byte aligned whenever the array does");

// the simulator's rule for one side: so / le = the masks "bin > up" / "bin <= down" of the 21 nodes -> the visited decided nodes, the
// visited edge nodes and checked[0..3] (k_sim_eval, gates none)
__device__ __forceinline__ void descend(unsigned so, unsigned le, unsigned inside, unsigned edge, unsigned corner, unsigned& dec, unsigned& edg,
                                        unsigned chk[4]) {
    const unsigned co = le & ~so;
    const unsigned rec = (inside & ~co) | edge;  // a visited node with this bit visits its sub-CUs
    unsigned vis = 1u | ((0u - (rec & 1u)) & kL1);
    const unsigned t = (rec & vis) >> 1 & 0xfu, x = (t | t << 3 | t << 6 | t << 9) & 0x1111u;
    vis |= (x * 15u) << 5;
    dec = vis & inside;
    edg = vis & edge;
    const unsigned checked = dec & ~so;  // CURRENT ONLY and BOTH
    chk[0] = checked & 1u;
    chk[1] = __popc(checked & kL1);
    chk[2] = __popc(checked & kL2);
    // 8 x 8 CUs: four under a recursing 16 x 16 node, two (one in the corner) under an edge node
    chk[3] = 4u * __popc(dec & rec & kL2) + 2u * __popc(edg & kL2) - __popc(edg & corner);
}

// A whole tile of 16-byte aligned arrays is kVec = 1344 float4 a side: five per lane and a sixth in the first wave.  Named registers, not
// an array: the loads of the NEXT tile stay in flight across the compare of this one.
constexpr int kVec = kTile * kNout / 4;
static_assert(kVec > 5 * kThreads && kVec <= 6 * kThreads, "five loads a lane and a tail");
typedef float v4f __attribute__((ext_vector_type(4)));
struct TileRegs {
    v4f a0, a1, a2, a3, a4, a5, b0, b1, b2, b3, b4, b5;
};
__device__ __forceinline__ void fetch(const float* __restrict__ a, const float* __restrict__ b, long tile, int t, TileRegs& r) {
    const v4f *pa = reinterpret_cast<const v4f*>(a + tile * kTile * kNout) + t, *pb = reinterpret_cast<const v4f*>(b + tile * kTile * kNout) + t;
    r.a0 = pa[0];
    r.b0 = pb[0];
    r.a1 = pa[kThreads];
    r.b1 = pb[kThreads];
    r.a2 = pa[2 * kThreads];
    r.b2 = pb[2 * kThreads];
    r.a3 = pa[3 * kThreads];
    r.b3 = pb[3 * kThreads];
    r.a4 = pa[4 * kThreads];
    r.b4 = pb[4 * kThreads];
    if (t + 5 * kThreads < kVec) {
        r.a5 = pa[5 * kThreads];
        r.b5 = pb[5 * kThreads];
    }
}
__device__ __forceinline__ void stage(float* s_a, float* s_b, int t, const TileRegs& r) {
    v4f *qa = reinterpret_cast<v4f*>(s_a) + t, *qb = reinterpret_cast<v4f*>(s_b) + t;
    qa[0] = r.a0;
    qb[0] = r.b0;
    qa[kThreads] = r.a1;
    qb[kThreads] = r.b1;
    qa[2 * kThreads] = r.a2;
    qb[2 * kThreads] = r.b2;
    qa[3 * kThreads] = r.a3;
    qb[3 * kThreads] = r.b3;
    qa[4 * kThreads] = r.a4;
    qb[4 * kThreads] = r.b4;
    if (t + 5 * kThreads < kVec) {
        qa[5 * kThreads] = r.a5;
        qb[5 * kThreads] = r.b5;
    }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
        v += (unsigned long long)hi << 32 | lo;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
        const unsigned long long w = (unsigned long long)hi << 32 | lo;
        v = v > w ? v : w;
    }
    return v;
}

// A block stages kTile CTUs of both sides per trip (contiguous floats in either layout: 16-byte loads through registers when both arrays
// are 16-byte aligned, dword loads else), then lane t compares CTU t of the tile.  A lane keeps its sums in registers over all its trips; a wave
// reduces them once, at the end, into the block's LDS words, and the block issues one atomic per non-zero word.
__global__ __launch_bounds__(kThreads) void k_compare(const float* __restrict__ a, const float* __restrict__ b, long n, long first, Geom g, float tol,
                                                      Thr thr, int vec, unsigned long long* __restrict__ words, uint8_t* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) float s_a[kTile * kNout];
    __shared__ __attribute__((aligned(16))) float s_b[kTile * kNout];
    __shared__ unsigned long long s_words[kWords];
    const int t = threadIdx.x;
    if (t < kWords) s_words[t] = 0ull;
    __syncthreads();
    unsigned sum[kSums];
#pragma unroll
    for (int i = 0; i < kSums; ++i) sum[i] = 0u;
    unsigned long long best[3] = {0ull, 0ull, 0ull};
    const long ntiles = (n + kTile - 1) / kTile;
    const long per = (long)g.ctus_w * g.ctus_h;
    // The loads of a whole tile of 16-byte aligned arrays are all issued before the first is waited for, and the NEXT tile's are issued
    // before this tile is compared, so the compare runs under the loads.  A partial tile (the last one) and arrays that are only 4-byte aligned take the plain loops.
    TileRegs regs;
    bool fetched = false;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long base = tile * kTile;
        const int cur = (int)(n - base < kTile ? n - base : kTile);
        if (vec && cur == kTile) {
            if (!fetched) fetch(a, b, tile, t, regs);
            stage(s_a, s_b, t, regs);
        } else {
            const int nf = cur * kNout;
            const float *src_a = a + base * kNout, *src_b = b + base * kNout;
            for (int i = t; i < nf; i += kThreads) {
                s_a[i] = src_a[i];
                s_b[i] = src_b[i];
            }
        }
        __syncthreads();
        const long next = tile + gridDim.x;
        fetched = vec && next < ntiles && n - next * kTile >= kTile;  // (uniform over the block)
        if (fetched) fetch(a, b, next, t, regs);
        if (t < cur) {
            const long ctu = first + base + t;
            unsigned inside = kAll, edge = 0u, corner = 0u;
            if (g.ctus_w) {  // the part rw x rh of the CTU inside the picture -> the geometry masks of k_sim_pack
                const int rem = (int)(ctu % per), cy = rem / g.ctus_w, cx = rem - cy * g.ctus_w;
                const int rw = g.width - 64 * cx < 64 ? g.width - 64 * cx : 64, rh = g.height - 64 * cy < 64 ? g.height - 64 * cy : 64;
                if (rw < 64 || rh < 64) {
                    inside = 0u;
#pragma unroll
                    for (int k = 0; k < kNout; ++k) {
                        const int q = k - 5, j = k < 5 ? k - 1 : q >> 2, i = q & 3;
                        const int bx = k == 0 ? 0 : k < 5 ? j & 1 : 2 * (j & 1) + (i & 1), by = k == 0 ? 0 : k < 5 ? j >> 1 : 2 * (j >> 1) + (i >> 1);
                        const int s = k == 0 ? 64 : k < 5 ? 32 : 16, ox = bx * s, oy = by * s;
                        if (ox + s <= rw && oy + s <= rh) inside |= 1u << k;
                        else if (ox < rw && oy < rh) {
                            edge |= 1u << k;
                            if (k >= 5 && rw - ox < 16 && rh - oy < 16) corner |= 1u << k;
                        }
                    }
                }
            }
            bool rejected = false;
            unsigned over[3] = {0u, 0u, 0u}, bdiff[3] = {0u, 0u, 0u}, top[3] = {0u, 0u, 0u};
            unsigned so_a = 0u, le_a = 0u, so_b = 0u, le_b = 0u;
#pragma unroll
            for (int k = 0; k < kNout; ++k) {
                // node k: its level and its raster index among the 21 probabilities
                const int q = k - 5, j = k < 5 ? k - 1 : q >> 2, i = q & 3;
                const int bx = k < 5 ? j & 1 : 2 * (j & 1) + (i & 1), by = k < 5 ? j >> 1 : 2 * (j >> 1) + (i >> 1);
                const int l = k == 0 ? 0 : k < 5 ? 1 : 2, r = k == 0 ? 0 : k < 5 ? 1 + bx + 2 * by : 5 + bx + 4 * by;
                const float x = s_a[t * kNout + r], y = s_b[t * kNout + r];
                const unsigned xb = __float_as_uint(x), yb = __float_as_uint(y);
                if ((xb > 0x3f800000u && xb != 0x80000000u) || (yb > 0x3f800000u && yb != 0x80000000u)) rejected = true;  // NaN, below 0, above 1
                const float d = x - y;                                // the one float operation
                const unsigned db = __float_as_uint(d) & 0x7fffffffu;  // |d|: orders as an integer
                over[l] += __uint_as_float(db) > tol ? 1u : 0u;
                bdiff[l] += xb != yb ? 1u : 0u;
                top[l] = top[l] > db ? top[l] : db;
                if (thr.has_thr) {  // bins with the bit tests of k_calib_count: p > 0 never lands in bin 0, whatever the denormal mode
                    int bin_a = (int)ceilf(x * 1024.f), bin_b = (int)ceilf(y * 1024.f);
                    if (bin_a == 0 && (xb & 0x7fffffffu)) bin_a = 1;
                    if (bin_b == 0 && (yb & 0x7fffffffu)) bin_b = 1;
                    const int up = thr.up[l], down = thr.down[l];
                    so_a |= (bin_a > up ? 1u : 0u) << k;
                    le_a |= (bin_a <= down ? 1u : 0u) << k;
                    so_b |= (bin_b > up ? 1u : 0u) << k;
                    le_b |= (bin_b <= down ? 1u : 0u) << k;
                }
            }
            unsigned f = 1u;
            if (rejected) {
                sum[kRejected] += 1u;
            } else {
                const unsigned low = ~(unsigned)ctu;  // ctu < 2^31: never 0, and the lower index is the larger word
                f = (over[0] | over[1] | over[2]) ? 2u : 0u;
#pragma unroll
                for (int l = 0; l < 3; ++l) {
                    sum[kOverTol + l] += over[l];
                    sum[kBitsDiff + l] += bdiff[l];
                    const unsigned long long v = (unsigned long long)top[l] << 32 | low;
                    best[l] = best[l] > v ? best[l] : v;
                }
                if (thr.has_thr) {
                    const unsigned cls = (so_a ^ so_b) | ((le_a & ~so_a) ^ (le_b & ~so_b));  // the outcome differs
                    sum[kClassDiff] += cls & 1u;
                    sum[kClassDiff + 1] += __popc(cls & kL1);
                    sum[kClassDiff + 2] += __popc(cls & kL2);
                    unsigned dec_a, edg_a, dec_b, edg_b, chk_a[4], chk_b[4];
                    descend(so_a, le_a, inside, edge, corner, dec_a, edg_a, chk_a);
                    descend(so_b, le_b, inside, edge, corner, dec_b, edg_b, chk_b);
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        sum[kCheckedA + d] += chk_a[d];
                        sum[kCheckedB + d] += chk_b[d];
                    }
                    // the sets of (visited node, outcome) differ: another node is visited, or a visited decided node has another outcome
                    const bool search = (dec_a | edg_a) != (dec_b | edg_b) || (dec_a & cls) != 0u;
                    sum[kSearchDiff] += search ? 1u : 0u;
                    f |= (cls ? 4u : 0u) | (search ? 8u : 0u);
                }
            }
            if (flags) flags[base + t] = (uint8_t)f;
        }
        __syncthreads();  // the next trip overwrites the staging
    }
#pragma unroll
    for (int i = 0; i < kSums; ++i) {
        const unsigned long long v = wave_sum(sum[i]);
        if ((t & 63) == 0 && v) atomicAdd(&s_words[i], v);
    }
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const unsigned long long v = wave_max(best[l]);
        if ((t & 63) == 0 && v) atomicMax(&s_words[kMax + l], v);
    }
    __syncthreads();
    if (t < kWords) {
        const unsigned long long v = s_words[t];
        if (v) {
            if (t < kSums) atomicAdd(&words[t], v);
            else atomicMax(&words[t], v);
        }
    }
}
}  // namespace

void launch_compare(hipStream_t s, const float* a, const float* b, long n, long first, const Geom& g, float tol, const Thr& thr,
                    unsigned long long* words, uint8_t* flags, int cus) {
    if (n <= 0) return;
    const int vec = (reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) % 16 == 0;
    k_compare<<<grid_for(n, cus), kThreads, 0, s>>>(a, b, n, first, g, tol, thr, vec, words, flags);
}

}  // namespace audit
}  // namespace ethcnn
