// ethcnn_lstm_samples_kernels.hip -- the ETH-LSTM sample-set kernels (launch list: ethcnn_lstm_samples.h; layouts: include/ethcnn.h
// "ETH-LSTM sample sets").  They move bytes: the only arithmetic is addresses and the uint8 -> float conversion of 17 bytes per time
// slot; no atomics, every output byte is written exactly once and never read back.
#include <hip/hip_runtime.h>

#include "ethcnn_lstm_samples.h"

namespace ethcnn {
namespace lstm_samples {

using train::kSlotBase;
using train::kSlotBytes;

namespace {
constexpr int kThreads = 256;
constexpr int kOutWords = kRecOut / 4;  // 9316
constexpr int kInfoWords = 16;
constexpr int kFlight = 4;              // dwords a lane of the gather has in flight

__global__ __launch_bounds__(kThreads) void k_lstm_headers(const uint8_t* __restrict__ rec, long nrec, Header* __restrict__ out) {
    for (long r = (long)blockIdx.x * kThreads + threadIdx.x; r < nrec; r += (long)gridDim.x * kThreads) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(rec + r * (long)kRecIn);  // (a record starts on a word)
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
        Header h;
        h.wh = w0 >> 16 | w1 << 16;       // bytes 2-3 | 4-5
        h.i_frame = w2 >> 16 | w3 << 16;  // bytes 10-13
        out[r] = h;
    }
}

// 16 aligned source bytes at p; only whole dwords below `end` exist (p and end are dword multiples)
__device__ __forceinline__ uint4 load16_below(const uint8_t* p, const uint8_t* end) {
    if (p + 16 <= end) return *reinterpret_cast<const uint4*>(p);
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = p + 4 * i + 4 <= end ? reinterpret_cast<const uint32_t*>(p)[i] : 0u;
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// 16 bytes out of the two aligned words around them; Q = whole dwords, sh = bits the first byte lies behind a 16-byte boundary
template <int Q>
__device__ __forceinline__ uint4 shift16(const uint4 a, const uint4 b, int sh) {
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = sh ? (w[Q + i] >> sh | w[Q + i + 1] << (32 - sh)) : w[Q + i];
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// CTU j of the chunk = record first + j; lane t carries bytes [16 t, 16 t + 16) of its residual = row t / 4, 16-byte column t % 4.
__global__ __launch_bounds__(kThreads) void k_resi_repack(const uint8_t* __restrict__ rec, long nrec, long first, int n, int slot,
                                                          uint8_t* __restrict__ picture) {
    const int t = threadIdx.x, row = t >> 2, c16 = (t & 3) * 16;
    const int total = (n + kTileCols - 1) / kTileCols * kTileCols;
    const uint8_t* end = rec + nrec * (long)kRecIn;
    for (int j = blockIdx.x; j < total; j += gridDim.x) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (j < n) {
            const uint8_t* src = rec + (first + j) * (long)kRecIn + kSlotBase + (long)kSlotBytes * slot + kGroup + 16 * t;
            const uintptr_t at = reinterpret_cast<uintptr_t>(src);
            const uint8_t* p = src - (at & 15);
            const int q = (int)(at & 15) >> 2, sh = (int)(at & 3) * 8;  // block-uniform: every lane's address is 16 t further
            const uint4 a = *reinterpret_cast<const uint4*>(p), b = load16_below(p + 16, end);
            v = q == 0 ? shift16<0>(a, b, sh) : q == 1 ? shift16<1>(a, b, sh) : q == 2 ? shift16<2>(a, b, sh) : shift16<3>(a, b, sh);
        }
        *reinterpret_cast<uint4*>(picture + ((long)(j / kTileCols) * 64 + row) * kPitch + (j % kTileCols) * 64 + c16) = v;
    }
}

__global__ __launch_bounds__(kThreads) void k_lstm_sample_gather(const uint8_t* __restrict__ rec, const float* __restrict__ vec,
                                                                 const int64_t* __restrict__ heads, const int64_t* __restrict__ strides,
                                                                 long m, int slot, uint8_t* __restrict__ out) {
    const int t = threadIdx.x;
    const uint32_t* vw = reinterpret_cast<const uint32_t*>(vec);
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const long head = heads[j], stride = strides[j];
        uint32_t* dst = reinterpret_cast<uint32_t*>(out + j * (long)kRecOut);
        for (int d0 = t; d0 < kOutWords; d0 += kFlight * kThreads) {
            uint32_t v[kFlight];
#pragma unroll
            for (int u = 0; u < kFlight; ++u) {
                const int d = d0 + u * kThreads;
                if (d >= kOutWords) continue;
                if (d < kInfoWords) {
                    const uint32_t w = reinterpret_cast<const uint32_t*>(rec + head * (long)kRecIn)[d];
                    v[u] = d == 0 ? ((w & ~255u) | (uint32_t)(kSteps - 1)) : w;
                } else {
                    const int k = (d - kInfoWords) / kSlotFloats, c = (d - kInfoWords) - k * kSlotFloats;
                    const long ref = head - k * stride;
                    if (c < kGroup) v[u] = __float_as_uint((float)rec[ref * (long)kRecIn + kSlotBase + (long)kSlotBytes * slot + c]);
                    else v[u] = vw[ref * (long)kVec + (c - kGroup)];
                }
            }
#pragma unroll
            for (int u = 0; u < kFlight; ++u) {
                const int d = d0 + u * kThreads;
                if (d < kOutWords) dst[d] = v[u];
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_lstm_qp0(const uint8_t* __restrict__ samples, long n, float* __restrict__ qp0) {
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads)
        qp0[i] = *reinterpret_cast<const float*>(samples + i * (long)kRecOut + 64);
}

__global__ __launch_bounds__(kThreads) void k_lstm_compact(const uint4* __restrict__ in, const int64_t* __restrict__ keep, long n,
                                                           uint4* __restrict__ out) {
    constexpr int kV = kRecOut / 16;  // 2329
    for (long j = blockIdx.x; j < n; j += gridDim.x) {
        const uint4* s = in + keep[j] * (long)kV;
        uint4* d = out + j * (long)kV;
        for (int k = threadIdx.x; k < kV; k += kThreads) d[k] = s[k];
    }
}

// the yardstick: a float4 grid-stride copy
__global__ __launch_bounds__(kThreads) void k_copy16(const float4* __restrict__ in, float4* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) out[i] = in[i];
}

int blocks_for(long want, int cus) { return (int)(want < (long)cus * 8 ? want : (long)cus * 8); }
}  // namespace

void launch_headers(hipStream_t s, const uint8_t* rec, long nrec, Header* out, int cus) {
    if (nrec <= 0) return;
    hipLaunchKernelGGL(k_lstm_headers, dim3(blocks_for((nrec + kThreads - 1) / kThreads, cus)), dim3(kThreads), 0, s, rec, nrec, out);
}

void launch_repack(hipStream_t s, const uint8_t* rec, long nrec, long first, int n, int slot, uint8_t* picture, int cus) {
    if (n <= 0) return;
    const int total = (n + kTileCols - 1) / kTileCols * kTileCols;
    hipLaunchKernelGGL(k_resi_repack, dim3(blocks_for(total, cus)), dim3(kThreads), 0, s, rec, nrec, first, n, slot, picture);
}

void launch_sample_gather(hipStream_t s, const uint8_t* rec, const float* vec, const int64_t* heads, const int64_t* strides, long m, int slot,
                          uint8_t* out, int cus) {
    if (m <= 0) return;
    hipLaunchKernelGGL(k_lstm_sample_gather, dim3(blocks_for(m, cus)), dim3(kThreads), 0, s, rec, vec, heads, strides, m, slot, out);
}

void launch_qp0(hipStream_t s, const uint8_t* samples, long n, float* qp0) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_lstm_qp0, dim3(blocks_for((n + kThreads - 1) / kThreads, 256)), dim3(kThreads), 0, s, samples, n, qp0);
}

void launch_compact(hipStream_t s, const uint8_t* in, const int64_t* keep, long n, uint8_t* out, int cus) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_lstm_compact, dim3(blocks_for(n, cus)), dim3(kThreads), 0, s, reinterpret_cast<const uint4*>(in), keep, n,
                       reinterpret_cast<uint4*>(out));
}

void launch_copy16(hipStream_t s, const uint8_t* in, uint8_t* out, long nbytes, int cus) {
    if (nbytes < 16) return;
    hipLaunchKernelGGL(k_copy16, dim3(blocks_for((nbytes / 16 + kThreads - 1) / kThreads, cus)), dim3(kThreads), 0, s,
                       reinterpret_cast<const float4*>(in), reinterpret_cast<float4*>(out), nbytes / 16);
}

}  // namespace lstm_samples
}  // namespace ethcnn
