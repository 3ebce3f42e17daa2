// ethcnn_replay.hip -- the sample-set replay kernels (launch list: ethcnn_replay.h; definitions: include/ethcnn.h "sample-set replay").
// They move bytes: no arithmetic beyond addresses and funnel shifts, no atomics, every plane byte is written exactly once and never read
// back.
#include <hip/hip_runtime.h>

#include "ethcnn_replay.h"

namespace ethcnn {
namespace replay {

using train::kSlotBase;
using train::kSlotBytes;

namespace {
constexpr int kThreads = 256;
constexpr int kFlight = 2;  // CTUs a block has in flight

// byte b of a record out of its aligned words
__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int b) { return (w[b >> 2] >> ((b & 3) * 8)) & 255u; }

__global__ __launch_bounds__(kThreads) void k_replay_headers(const uint8_t* __restrict__ rec, long nrec, Header* __restrict__ out) {
    for (long r = (long)blockIdx.x * kThreads + threadIdx.x; r < nrec; r += (long)gridDim.x * kThreads) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(rec + r * (long)kRec);  // (a record starts on a word)
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
        Header h;
        h.wh = w0 >> 16 | w1 << 16;       // bytes 2-3 | 4-5
        h.f = w2 >> 16 | w3 << 16;        // bytes 10-13
        h.linecol = w3 >> 16 | w4 << 16;  // bytes 14-15 | 16-17
        h.seq = w4 >> 16;                 // bytes 18-19
        h.qps = byte_of(w, kSlotBase) | byte_of(w, kSlotBase + kSlotBytes) << 8 | byte_of(w, kSlotBase + 2 * kSlotBytes) << 16 |
                byte_of(w, kSlotBase + 3 * kSlotBytes) << 24;
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

// 16 bytes out of the two aligned words around them; Q = whole dwords, sh = bits the first byte lies behind a dword boundary
template <int Q>
__device__ __forceinline__ uint4 shift16(const uint4 a, const uint4 b, int sh) {
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = sh ? (w[Q + i] >> sh | w[Q + i + 1] << (32 - sh)) : w[Q + i];
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// entry j of src = (frame j / nctu, CTU j % nctu in raster order); lane t carries bytes [16 t, 16 t + 16) of the record's residual = row
// t / 4, 16-byte column t % 4 of the CTU; lanes 0..3 also row t of its 4 x 4 depth map.
__global__ __launch_bounds__(kThreads) void k_uncut_inter(const uint8_t* __restrict__ rec, long nrec, const int64_t* __restrict__ src, long total,
                                                          int nctu, int C, int slot, uint8_t* __restrict__ resi, uint8_t* __restrict__ labels) {
    const int t = threadIdx.x, row = t >> 2, c16 = (t & 3) * 16;
    const uint8_t* end = rec + nrec * (long)kRec;
    const long stride = gridDim.x;
    for (long j0 = blockIdx.x; j0 < total; j0 += kFlight * stride) {
        uint4 v[kFlight];
        uint32_t lab[kFlight];
#pragma unroll
        for (int u = 0; u < kFlight; ++u) {
            const long j = j0 + u * stride;
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            lab[u] = 0u;
            if (j >= total) continue;
            const long idx = src[j];
            if (idx < 0 || idx >= nrec) continue;  // (a table the caller built: nothing outside the buffer is read)
            const uint8_t* slot0 = rec + idx * (long)kRec + kSlotBase + (long)kSlotBytes * slot;  // the slot's QP byte
            const uintptr_t at = reinterpret_cast<uintptr_t>(slot0 + kGroup);
            const int off = __builtin_amdgcn_readfirstlane((int)(at & 15));  // block-uniform: every lane's address is 16 t further
            const uint8_t* p = slot0 + kGroup - off + 16 * t;
            const int q = off >> 2, sh = (off & 3) * 8;
            const uint4 a = *reinterpret_cast<const uint4*>(p);
            uint4 b = make_uint4(0u, 0u, 0u, 0u);
            if (off) b = load16_below(p + 16, end);
            v[u] = q == 0 ? shift16<0>(a, b, sh) : q == 1 ? shift16<1>(a, b, sh) : q == 2 ? shift16<2>(a, b, sh) : shift16<3>(a, b, sh);
            if (t < 4) {
                const uint8_t* lp = slot0 + 1 + 4 * t;
                const int lsh = (int)(reinterpret_cast<uintptr_t>(lp) & 3) * 8;
                const uint32_t* lw = reinterpret_cast<const uint32_t*>(lp - (lsh >> 3));
                const uint32_t w0 = lw[0];
                lab[u] = lsh ? (w0 >> lsh | lw[1] << (32 - lsh)) : w0;  // (lw[1] is inside the record: the residual follows)
            }
        }
#pragma unroll
        for (int u = 0; u < kFlight; ++u) {
            const long j = j0 + u * stride;
            if (j >= total) continue;
            const long f = j / nctu;
            const int ctu = (int)(j - f * nctu), line = ctu / C, col = ctu - line * C;
            *reinterpret_cast<uint4*>(resi + f * 4096L * nctu + (long)(line * 64 + row) * (64 * C) + col * 64 + c16) = v[u];
            if (t < 4) *reinterpret_cast<uint32_t*>(labels + f * 16L * nctu + (long)(line * 4 + t) * (4 * C) + col * 4) = lab[u];
        }
    }
}

int blocks_for(long want, int cus) { return (int)(want < (long)cus * 8 ? want : (long)cus * 8); }
}  // namespace

void launch_headers(hipStream_t s, const uint8_t* rec, long nrec, Header* out, int cus) {
    if (nrec <= 0) return;
    hipLaunchKernelGGL(k_replay_headers, dim3(blocks_for((nrec + kThreads - 1) / kThreads, cus)), dim3(kThreads), 0, s, rec, nrec, out);
}

void launch_uncut(hipStream_t s, const uint8_t* rec, long nrec, const int64_t* src, long nframes, int R, int C, int slot, uint8_t* resi,
                  uint8_t* labels, int cus) {
    const long total = nframes * R * C;
    if (total <= 0) return;
    hipLaunchKernelGGL(k_uncut_inter, dim3(blocks_for((total + kFlight - 1) / kFlight, cus)), dim3(kThreads), 0, s, rec, nrec, src, total, R * C,
                       C, slot, resi, labels);
}

}  // namespace replay
}  // namespace ethcnn
