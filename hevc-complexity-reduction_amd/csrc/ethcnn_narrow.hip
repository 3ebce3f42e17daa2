// ethcnn_narrow.hip -- k_narrow_luma: 16-bit luma planes in HBM -> packed 8-bit planes (access pattern and launch: ethcnn_narrow.h;
// the rule: include/ethcnn.h "high-bit-depth and non-4:2:0 sources").  It moves bytes: two packed 16-bit operations and half a byte
// permute per sample pair, no LDS, no atomics, every output byte written exactly once.
#include <hip/hip_runtime.h>

#include "ethcnn_narrow.h"

namespace ethcnn {
namespace narrow {

namespace {
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kFlight = 2;  // units a wave has in flight (the loads of both before the stores of either)

// 16 source bytes at the 16-byte aligned p of a row of which `left` bytes (even; may be <= 0) lie at and behind p: whole dwords
// below the row's end, then one 16-bit load when it ends on half a dword; what does not exist reads as zero
__device__ __forceinline__ uint4 load16_left(const uint8_t* p, long left) {
    if (left >= 16) return *reinterpret_cast<const uint4*>(p);
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = 0u;
        if (left >= 4 * i + 4) w[i] = *reinterpret_cast<const uint32_t*>(p + 4 * i);
        else if (left >= 4 * i + 2) w[i] = *reinterpret_cast<const uint16_t*>(p + 4 * i);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// 32 source bytes (16 samples) out of the three aligned words around them -> 16 narrowed bytes; Q = whole dwords and half = whether
// a further 16 bits lie between the aligned boundary and the first sample
template <int Q>
__device__ __forceinline__ uint4 narrow16(const uint4 a, const uint4 b, const uint4 c, bool half, int shift) {
    const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    uint32_t s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = half ? (w[Q + i] >> 16 | w[Q + i + 1] << 16) : w[Q + i];
    return narrow8(s, shift);  // (ethcnn_narrow.h)
}

// unit u = (frame * height + row) * chunks + chunk: segments [64 chunk, 64 chunk + 64) of that row, one per lane
__global__ __launch_bounds__(kThreads) void k_narrow_luma(const uint8_t* __restrict__ src, int width, int height, long pitch, long fstride,
                                                          int units, int chunks, int shift, uint8_t* __restrict__ dst, long dpitch,
                                                          long dfstride) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nseg = (width + 15) >> 4;
    const long stride = (long)gridDim.x * kWaves;
    for (long u0 = (long)blockIdx.x * kWaves + wave; u0 < units; u0 += kFlight * stride) {
        uint4 v[kFlight];
        long at[kFlight];  // destination offset of the lane's 16 bytes; < 0: nothing to store
#pragma unroll
        for (int k = 0; k < kFlight; ++k) {
            const long u = u0 + k * stride;
            at[k] = -1;
            v[k] = make_uint4(0u, 0u, 0u, 0u);
            if (u >= units) continue;
            const int line = (int)u / chunks, chunk = (int)u - line * chunks;
            const int f = line / height, y = line - f * height;
            const int seg = chunk * 64 + lane;
            if (seg >= nseg) continue;
            const uint8_t* rowp = src + f * fstride + y * pitch;
            const int off = __builtin_amdgcn_readfirstlane((int)(reinterpret_cast<uintptr_t>(rowp) & 15));  // even; the same in every lane
            const uint8_t* p = rowp - off + 32L * seg;  // 16-byte aligned
            const long left = 2L * width + off - 32L * seg;  // bytes of the row at and behind p (> 0: seg < nseg)
            const uint4 a = load16_left(p, left), b = load16_left(p + 16, left - 16);
            uint4 c = make_uint4(0u, 0u, 0u, 0u);
            if (off) c = load16_left(p + 32, left - 32);
            const int q = off >> 2;
            const bool half = (off & 2) != 0;
            uint4 r = q == 0 ? narrow16<0>(a, b, c, half, shift) : q == 1 ? narrow16<1>(a, b, c, half, shift)
                    : q == 2 ? narrow16<2>(a, b, c, half, shift) : narrow16<3>(a, b, c, half, shift);
            const int valid = width - 16 * seg;  // samples of this segment inside the row; the rest of the 16 bytes is written as zero
            if (valid < 16) {
                uint32_t o[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int keep = valid - 4 * i;
                    o[i] = keep >= 4 ? o[i] : keep <= 0 ? 0u : (o[i] & ((1u << (8 * keep)) - 1u));
                }
                r = make_uint4(o[0], o[1], o[2], o[3]);
            }
            v[k] = r;
            at[k] = f * dfstride + y * dpitch + 16L * seg;
        }
#pragma unroll
        for (int k = 0; k < kFlight; ++k)
            if (at[k] >= 0) *reinterpret_cast<uint4*>(dst + at[k]) = v[k];
    }
}
}  // namespace

void launch_narrow(hipStream_t s, const uint8_t* src, int width, int height, long pitch, long fstride, int nframes, int shift, uint8_t* dst,
                   long dst_pitch, long dst_fstride, int cus) {
    const int chunks = ((width + 15) / 16 + 63) / 64;
    const long units = (long)nframes * height * chunks;  // (< 2^31: checked by the caller)
    if (units <= 0) return;
    const long want = (units + kWaves * kFlight - 1) / (kWaves * kFlight), cap = (long)(cus > 0 ? cus : 256) * 8;
    hipLaunchKernelGGL(k_narrow_luma, dim3((unsigned)(want < cap ? want : cap)), dim3(kThreads), 0, s, src, width, height, pitch, fstride,
                       (int)units, chunks, shift, dst, dst_pitch, dst_fstride);
}

}  // namespace narrow
}  // namespace ethcnn
