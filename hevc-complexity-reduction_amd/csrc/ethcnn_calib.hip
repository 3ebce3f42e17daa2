// ethcnn_calib.hip -- the calibration kernel (launch list and state layout: ethcnn_calib.h; definitions: include/ethcnn.h "threshold
// calibration").  Integer counting only: no float is accumulated anywhere, so the histogram is exact and independent of the schedule.
#include <hip/hip_runtime.h>

#include "ethcnn_calib.h"

namespace ethcnn {
namespace calib {

namespace {
constexpr int kThreads = 256;
constexpr int kNout = 21;
enum { kMiscRejected = 0, kMiscSkipped = 3, kMiscBad = 4, kMiscWords = 8 };

__device__ __forceinline__ unsigned sum4(unsigned w) { return (w & 0xffu) + (w >> 8 & 0xffu) + (w >> 16 & 0xffu) + (w >> 24); }

// one sample: its probability into the block's histogram of (level, truth), or into rejected[level].  The range test and the
// "p > 0 never lands in bin 0" rule are done on the bits, so they do not depend on the denormal mode the multiply runs in.
__device__ __forceinline__ void count(unsigned* hist, unsigned* misc, int level, bool truth, float p) {
    const unsigned bits = __float_as_uint(p);
    if (bits > 0x3f800000u && bits != 0x80000000u) {  // NaN, below 0, above 1 (-0 is 0)
        atomicAdd(&misc[kMiscRejected + level], 1u);
        return;
    }
    int bin = (int)ceilf(p * 1024.f);  // exact product, 0..1024
    if (bin == 0 && (bits & 0x7fffffffu)) bin = 1;
    atomicAdd(&hist[(level * 2 + (truth ? 1 : 0)) * kBins + bin], 1u);
}

// A block stages kTile CTUs per trip: their 21 probabilities (contiguous floats in either layout) and their 16 depth bytes as four
// row dwords (per-CTU layout: contiguous; frame layout: the four 4-byte rows of the CTU's 4 x 4 map out of the label plane).  Then
// lane (c, j) = (t / 4, t % 4) counts 32 x 32 block j of CTU c and its four 16 x 16 blocks; lane j == 0 also counts the CTU itself.
__global__ __launch_bounds__(kThreads) void k_calib_count(const float* __restrict__ probs, const uint8_t* __restrict__ labels, long n, Geom g,
                                                          int rows_aligned, unsigned long long* __restrict__ call) {
    __shared__ unsigned s_hist[kHistWords];
    __shared__ unsigned s_misc[kMiscWords];
    __shared__ float s_p[kTile * kNout];
    __shared__ unsigned s_d[kTile * 4];
    __shared__ unsigned s_whole[kTile];
    const int t = threadIdx.x;
    for (int i = t; i < kHistWords; i += kThreads) s_hist[i] = 0u;
    if (t < kMiscWords) s_misc[t] = 0u;
    __syncthreads();
    const long ntiles = (n + kTile - 1) / kTile;
    const long per = (long)g.ctus_w * g.ctus_h;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long base = tile * kTile;
        const int cur = (int)(n - base < kTile ? n - base : kTile);
        const float* src = probs + base * kNout;
        for (int i = t; i < cur * kNout; i += kThreads) s_p[i] = src[i];
        if (t < cur * 4) {
            const int c = t >> 2, r = t & 3;
            unsigned w = 0u, whole = 1u;
            if (g.ctus_w == 0) {
                w = reinterpret_cast<const unsigned*>(labels)[base * 4 + t];
            } else {
                const long ctu = base + c, f = ctu / per;
                const int rem = (int)(ctu - f * per), cy = rem / g.ctus_w, cx = rem - cy * g.ctus_w;
                whole = cx < g.whole_w && cy < g.whole_h ? 1u : 0u;
                if (whole) {  // rows 4 cy + r < h16 and columns 4 cx + 3 < w16 of label frame f
                    const uint8_t* q = labels + ((f * g.h16 + cy * 4 + r) * (long)g.w16 + cx * 4);
                    w = rows_aligned ? *reinterpret_cast<const unsigned*>(q)
                                     : (unsigned)q[0] | (unsigned)q[1] << 8 | (unsigned)q[2] << 16 | (unsigned)q[3] << 24;
                }
            }
            s_d[t] = w;
            if (r == 0) s_whole[c] = whole;
        }
        __syncthreads();
        if (t < cur * 4) {
            const int c = t >> 2, j = t & 3;
            if (!s_whole[c]) {
                if (j == 0) atomicAdd(&s_misc[kMiscSkipped], 1u);
            } else {
                const unsigned d0 = s_d[c * 4], d1 = s_d[c * 4 + 1], d2 = s_d[c * 4 + 2], d3 = s_d[c * 4 + 3];
                if ((d0 | d1 | d2 | d3) & 0xfcfcfcfcu) {
                    if (j == 0) atomicAdd(&s_misc[kMiscBad], 1u);  // a depth above 3: the whole call will add nothing
                } else {
                    const float* p = s_p + c * kNout;
                    const bool t64 = sum4(d0) + sum4(d1) + sum4(d2) + sum4(d3) > 8u;
                    if (j == 0) count(s_hist, s_misc, 0, t64, p[0]);
                    if (t64) {
                        const int qy = j >> 1, qx = j & 1;
                        const unsigned a = (qy ? d2 : d0) >> (16 * qx) & 0xffffu, b = (qy ? d3 : d1) >> (16 * qx) & 0xffffu;
                        const unsigned b0 = a & 0xffu, b1 = a >> 8, b2 = b & 0xffu, b3 = b >> 8;
                        const bool t32 = b0 + b1 + b2 + b3 > 6u;
                        count(s_hist, s_misc, 1, t32, p[1 + j]);
                        if (t32) {
                            const float* p16 = p + 5 + 8 * qy + 2 * qx;  // IDX32[j] = first + {0, 1, 4, 5}
                            count(s_hist, s_misc, 2, b0 == 3u, p16[0]);
                            count(s_hist, s_misc, 2, b1 == 3u, p16[1]);
                            count(s_hist, s_misc, 2, b2 == 3u, p16[4]);
                            count(s_hist, s_misc, 2, b3 == 3u, p16[5]);
                        }
                    }
                }
            }
        }
        __syncthreads();  // the next trip overwrites the staging
    }
    for (int i = t; i < kHistWords; i += kThreads) {
        const unsigned v = s_hist[i];
        if (v) atomicAdd(&call[i], (unsigned long long)v);
    }
    if (t < 3 && s_misc[kMiscRejected + t]) atomicAdd(&call[kRejected + t], (unsigned long long)s_misc[kMiscRejected + t]);
    if (t == 3 && s_misc[kMiscSkipped]) atomicAdd(&call[kSkipped], (unsigned long long)s_misc[kMiscSkipped]);
    if (t == 4 && s_misc[kMiscBad]) atomicAdd(&call[kFlag], (unsigned long long)s_misc[kMiscBad]);
}

// acc += call unless the flag is up; call = 0 either way (the flag word itself is zeroed by the host before the next count)
__global__ __launch_bounds__(kThreads) void k_calib_commit(unsigned long long* __restrict__ acc, unsigned long long* __restrict__ call) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= kWords) return;
    const unsigned long long v = call[i];
    if (call[kFlag] == 0ull && v) acc[i] += v;
    call[i] = 0ull;
}
}  // namespace

void launch_count(hipStream_t s, const float* probs, const uint8_t* labels, long n, const Geom& g, unsigned long long* call, int cus) {
    if (n <= 0) return;
    const long ntiles = (n + kTile - 1) / kTile;
    const int grid = (int)(ntiles < 4L * cus ? ntiles : 4L * cus);
    const int rows_aligned = g.ctus_w != 0 && g.w16 % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % 4 == 0;
    k_calib_count<<<grid, kThreads, 0, s>>>(probs, labels, n, g, rows_aligned, call);
}

void launch_commit(hipStream_t s, unsigned long long* acc, unsigned long long* call) {
    k_calib_commit<<<(kWords + kThreads - 1) / kThreads, kThreads, 0, s>>>(acc, call);
}

}  // namespace calib
}  // namespace ethcnn
