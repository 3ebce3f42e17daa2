// ethcnn_samples_kernels.hip -- the sample-set kernels (launch list: ethcnn_samples.h; record layouts: include/ethcnn.h "sample sets").
// They move bytes: no arithmetic beyond addresses (k_cut_ai16: and the narrowing rule), no atomics, every byte of a record is written
// exactly once and never read back.
#include <hip/hip_runtime.h>

#include "ethcnn_narrow.h"
#include "ethcnn_samples.h"

namespace ethcnn {
namespace samples {

using train::kLabelBase;
using train::kRec;
using train::kRecLdp;
using train::kSlotBase;
using train::kSlotBytes;

namespace {
constexpr int kThreads = 256;
constexpr int kRecWords = kRecLdp / 4;  // 4129

// 16 consecutive source bytes; A = what the address is known to be a multiple of
template <int A>
__device__ __forceinline__ uint4 load16(const uint8_t* p) {
    if (A == 16) return *reinterpret_cast<const uint4*>(p);
    uint32_t w[4];
    if (A == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = reinterpret_cast<const uint32_t*>(p)[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint32_t load4(const uint8_t* p, int al4) {
    if (al4) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

struct Where {
    long f;
    int cl, cc;
};
__device__ __forceinline__ Where locate(const CutArgs& a, long r) {
    const long per = (long)a.nl * a.nc;
    Where w;
    w.f = r / per;
    const int c = (int)(r - w.f * per);
    w.cl = c / a.nc;
    w.cc = c - w.cl * a.nc;
    return w;
}

// All-Intra: 4992 bytes = 312 x 16.  Lanes 0..255 carry the luma tile (row = lane / 4, 16-byte column = lane % 4); lanes 0..55 also the
// tail: dwordx4 words 256..259 = the 64 fill bytes, word 260 + q = the label row of QP q (the CTU's 4 x 4 depths, four 4-byte runs of the
// label plane).  Two records per trip, loads of both before the stores of either.
template <int A>
__global__ __launch_bounds__(kThreads) void k_cut_ai(const CutArgs a) {
    const int t = threadIdx.x, row = t >> 2, c16 = (t & 3) * 16;
    const long stride = gridDim.x;
    for (long r0 = blockIdx.x; r0 < a.nrec; r0 += 2 * stride) {
        uint4 v[2], tail[2];
        bool on[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long r = r0 + u * stride;
            on[u] = r < a.nrec;
            if (!on[u]) continue;
            const Where w = locate(a, r);
            v[u] = load16<A>(a.luma[0] + w.f * a.fstride[0] + (long)(w.cl * 64 + row) * a.pitch[0] + w.cc * 64 + c16);
            tail[u] = make_uint4(~0u, ~0u, ~0u, ~0u);
            if (t >= 4 && t < 56 && a.label[t - 4]) {
                const uint8_t* lp = a.label[t - 4] + w.f * a.label_fstride + (long)(w.cl * 4) * a.lw + w.cc * 4;
                tail[u] = make_uint4(load4(lp, a.label_al4), load4(lp + a.lw, a.label_al4), load4(lp + 2 * a.lw, a.label_al4),
                                     load4(lp + 3 * a.lw, a.label_al4));
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!on[u]) continue;
            uint4* dst = reinterpret_cast<uint4*>(a.out + (r0 + u * stride) * (long)kRec);
            dst[t] = v[u];
            if (t < 56) dst[256 + t] = tail[u];
        }
    }
}

// 32 consecutive source bytes = 16 samples of 16 bits; A = what the address is known to be a multiple of (16, 4 or 2)
template <int A>
__device__ __forceinline__ void load32(const uint8_t* p, uint32_t (&w)[8]) {
    if (A == 16) {
        const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
        w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
    } else if (A == 4) {
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = reinterpret_cast<const uint32_t*>(p)[i];
    } else {
        const uint16_t* h = reinterpret_cast<const uint16_t*>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = (uint32_t)h[2 * i] | (uint32_t)h[2 * i + 1] << 16;
    }
}

// All-Intra from 16-bit luma: k_cut_ai with a deep source.  The same lane owns the same 16 samples of its tile row: 32 source bytes at
// byte column 128 cc + 32 (lane % 4) of row 64 cl + lane / 4, narrowed to the 16 record bytes by the rule (ethcnn_narrow.h).  Only whole
// CTUs are samples, so those 32 bytes always lie inside the row's 2 * width bytes: there is no edge path, and nothing is read outside
// rows [0, 64 (height / 64)) or outside columns [0, 64 (width / 64)) of a plane.  Record layout, tail, loop and stores as k_cut_ai; the
// loads of both records in flight are issued before the stores of either.
template <int A>
__global__ __launch_bounds__(kThreads) void k_cut_ai16(const CutArgs a) {
    const int t = threadIdx.x, row = t >> 2, c32 = (t & 3) * 32;
    const long stride = gridDim.x;
    for (long r0 = blockIdx.x; r0 < a.nrec; r0 += 2 * stride) {
        uint32_t v[2][8];
        uint4 tail[2];
        bool on[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long r = r0 + u * stride;
            on[u] = r < a.nrec;
            if (!on[u]) continue;
            const Where w = locate(a, r);
            load32<A>(a.luma[0] + w.f * a.fstride[0] + (long)(w.cl * 64 + row) * a.pitch[0] + w.cc * 128 + c32, v[u]);
            tail[u] = make_uint4(~0u, ~0u, ~0u, ~0u);
            if (t >= 4 && t < 56 && a.label[t - 4]) {
                const uint8_t* lp = a.label[t - 4] + w.f * a.label_fstride + (long)(w.cl * 4) * a.lw + w.cc * 4;
                tail[u] = make_uint4(load4(lp, a.label_al4), load4(lp + a.lw, a.label_al4), load4(lp + 2 * a.lw, a.label_al4),
                                     load4(lp + 3 * a.lw, a.label_al4));
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!on[u]) continue;
            uint4* dst = reinterpret_cast<uint4*>(a.out + (r0 + u * stride) * (long)kRec);
            dst[t] = narrow::narrow8(v[u], a.shift);
            if (t < 56) dst[256 + t] = tail[u];
        }
    }
}

// inter header byte i (extract_data_LDP_LDB_RA.py:131-146): little-endian fields, 255 elsewhere
__device__ __forceinline__ uint32_t header_byte(const CutArgs& a, int i, uint32_t frame, int cl, int cc) {
    switch (i) {
        case 0: return 1;
        case 2: return a.width & 255;
        case 3: return (a.width >> 8) & 255;
        case 4: return a.height & 255;
        case 5: return (a.height >> 8) & 255;
        case 10: return frame & 255;
        case 11: return (frame >> 8) & 255;
        case 12: return (frame >> 16) & 255;
        case 13: return frame >> 24;
        case 14: return cl & 255;
        case 15: return (cl >> 8) & 255;
        case 16: return cc & 255;
        case 17: return (cc >> 8) & 255;
        case 18: return a.seq & 255;
        case 19: return (a.seq >> 8) & 255;
        default: return 255;
    }
}

// inter: 16516 bytes = 4129 dwords.  Byte b of a record: b < 64 header; else slot s = (b - 64) / 4113, o = (b - 64) % 4113:
// o = 0 the QP, 1..16 the labels, 17.. the residual tile byte o - 17.
template <int A>
__global__ __launch_bounds__(kThreads) void k_cut_inter(const CutArgs a) {
    __shared__ uint4 tile[4][kThreads];                           // the four tiles, aligned
    __shared__ uint8_t meta[kHeaderBytes + 4 * kGroupBytes + 4];  // header | 4 x [QP | 16 labels]
    const int t = threadIdx.x, row = t >> 2, c16 = (t & 3) * 16;
    auto byte_at = [&](int b) -> uint32_t {
        if (b < kHeaderBytes) return meta[b];
        const int s = (b - kSlotBase) / kSlotBytes, o = (b - kSlotBase) - s * kSlotBytes;
        if (o < kGroupBytes) return meta[kHeaderBytes + s * kGroupBytes + o];
        return reinterpret_cast<const uint8_t*>(tile[s])[o - kGroupBytes];
    };
    for (long r = blockIdx.x; r < a.nrec; r += gridDim.x) {
        const Where w = locate(a, r);
        uint4 v[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) v[s] = load16<A>(a.luma[s] + w.f * a.fstride[s] + (long)(w.cl * 64 + row) * a.pitch[s] + w.cc * 64 + c16);
        uint32_t m = 0;
        if (t < kHeaderBytes) {
            m = header_byte(a, t, (uint32_t)(a.frame0 + w.f), w.cl, w.cc);
        } else if (t < kHeaderBytes + 4 * kGroupBytes) {
            const int s = (t - kHeaderBytes) / kGroupBytes, o = (t - kHeaderBytes) - s * kGroupBytes;
            m = o == 0 ? (uint32_t)a.qps[s]
                       : a.label[s][w.f * a.label_fstride + (long)(w.cl * 4 + ((o - 1) >> 2)) * a.lw + w.cc * 4 + ((o - 1) & 3)];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) tile[s][t] = v[s];
        if (t < kHeaderBytes + 4 * kGroupBytes) meta[t] = (uint8_t)m;
        __syncthreads();
        uint32_t* out = reinterpret_cast<uint32_t*>(a.out + r * (long)kRecLdp);
        for (int k = t; k < kRecWords; k += kThreads) {
            const int b = 4 * k;
            const int s = b < kSlotBase ? 0 : (b - kSlotBase) / kSlotBytes, o = (b - kSlotBase) - s * kSlotBytes;
            uint32_t word;
            if (b >= kSlotBase && o >= kGroupBytes && o + 3 < kSlotBytes) {  // four residual bytes of one slot: two aligned LDS words
                const int ti = o - kGroupBytes, sh = (ti & 3) * 8;
                const uint32_t* tw = reinterpret_cast<const uint32_t*>(tile[s]);
                word = tw[ti >> 2];
                if (sh) word = word >> sh | tw[(ti >> 2) + 1] << (32 - sh);
            } else {  // the header and the few words that touch a slot's QP / label group
                word = byte_at(b) | byte_at(b + 1) << 8 | byte_at(b + 2) << 16 | byte_at(b + 3) << 24;
            }
            out[k] = word;
        }
        __syncthreads();
    }
}

template <typename V>
__global__ __launch_bounds__(kThreads) void k_gather(const V* in, V* out, long first, long n, long count, int vecs, uint64_t seed,
                                                     int permuted) {
    for (long j = blockIdx.x; j < n; j += gridDim.x) {
        const long src = permuted ? (long)perm(seed, (uint64_t)count, (uint64_t)(first + j)) : first + j;
        const V* s = in + src * vecs;
        V* d = out + j * vecs;
        for (int k = threadIdx.x; k < vecs; k += kThreads) d[k] = s[k];
    }
}
}  // namespace

void launch_cut(hipStream_t s, int kind, const CutArgs& a, int align, int cus) {
    if (a.nrec <= 0) return;
    const long want = kind == kKindAi ? (a.nrec + 1) / 2 : a.nrec;
    const int blocks = (int)(want < (long)cus * 8 ? want : (long)cus * 8);
    if (kind == kKindAi && a.deep) {
        if (align >= 16) hipLaunchKernelGGL(k_cut_ai16<16>, dim3(blocks), dim3(kThreads), 0, s, a);
        else if (align >= 4) hipLaunchKernelGGL(k_cut_ai16<4>, dim3(blocks), dim3(kThreads), 0, s, a);
        else hipLaunchKernelGGL(k_cut_ai16<2>, dim3(blocks), dim3(kThreads), 0, s, a);
    } else if (kind == kKindAi) {
        if (align >= 16) hipLaunchKernelGGL(k_cut_ai<16>, dim3(blocks), dim3(kThreads), 0, s, a);
        else if (align >= 4) hipLaunchKernelGGL(k_cut_ai<4>, dim3(blocks), dim3(kThreads), 0, s, a);
        else hipLaunchKernelGGL(k_cut_ai<1>, dim3(blocks), dim3(kThreads), 0, s, a);
    } else {
        if (align >= 16) hipLaunchKernelGGL(k_cut_inter<16>, dim3(blocks), dim3(kThreads), 0, s, a);
        else if (align >= 4) hipLaunchKernelGGL(k_cut_inter<4>, dim3(blocks), dim3(kThreads), 0, s, a);
        else hipLaunchKernelGGL(k_cut_inter<1>, dim3(blocks), dim3(kThreads), 0, s, a);
    }
}

void launch_gather(hipStream_t s, int kind, const uint8_t* in, uint8_t* out, long first, long n, long count, uint64_t seed, int permuted,
                   int cus) {
    if (n <= 0) return;
    const int blocks = (int)(n < (long)cus * 8 ? n : (long)cus * 8);
    if (kind == kKindAi)
        hipLaunchKernelGGL(k_gather<uint4>, dim3(blocks), dim3(kThreads), 0, s, reinterpret_cast<const uint4*>(in),
                           reinterpret_cast<uint4*>(out), first, n, count, kRec / 16, seed, permuted);
    else
        hipLaunchKernelGGL(k_gather<uint32_t>, dim3(blocks), dim3(kThreads), 0, s, reinterpret_cast<const uint32_t*>(in),
                           reinterpret_cast<uint32_t*>(out), first, n, count, kRecLdp / 4, seed, permuted);
}

}  // namespace samples
}  // namespace ethcnn
