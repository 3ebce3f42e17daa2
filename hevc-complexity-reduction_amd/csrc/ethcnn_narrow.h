// ethcnn_narrow.h -- shared between the narrowing kernel (ethcnn_narrow.hip), its host side (ethcnn_narrow.cpp) and the host / file
// entries that narrow while they fill the staging ring (ethcnn_host.cpp): include/ethcnn.h "high-bit-depth and non-4:2:0 sources".
//
// The rule (stated once, in include/ethcnn.h): a deep sample is an unsigned 16-bit little-endian value s, and the network sees
// min(s >> (bit_depth - 8), 255), bit_depth 8..16.  shift = bit_depth - 8 everywhere below.
//
// k_narrow_luma: 16-bit luma planes in HBM -> packed 8-bit planes whose pitch is a multiple of 16 (roundup16(width) at least).
//   work unit   one wave per (frame, row, run of 64 segments); a segment = 16 output bytes = 32 source bytes; a lane owns one segment.
//               A row is the unit because the byte offset of a row's first sample from a 16-byte boundary (0, 2, .. 14: any even pitch
//               and any 2-byte aligned base are allowed) is then the same in every lane: the funnel shift amount is wave-uniform.
//   loads       two aligned dwordx4 loads around the lane's 32 bytes, a third one only when the row does not start on a 16-byte
//               boundary; 12 dwords -> 8 by a funnel shift of (offset / 4) whole dwords and 0 or 16 bits.  The aligned loads of the
//               first segment begin at the 16-byte boundary at or below the row's first sample (the same aligned line, never another
//               page); at the right edge nothing at or behind the row's last sample + 1 is read: whole dwords below it, then one
//               16-bit load when the row ends on half a dword.
//   arithmetic  per dword (two samples): packed 16-bit shift right by the uniform amount, packed 16-bit unsigned minimum with 255, and
//               one byte permute per output dword that picks the low bytes of four samples.
//   stores      one dwordx4 per lane; bytes [width, roundup16(width)) of a row are written as zero, nothing behind them is touched.
// No LDS, no atomics, every output byte has one writer.
//
// The device form of the rule (narrow2, pack4, narrow8 below) is shared with the deep cut kernel of the sample sets (k_cut_ai16,
// ethcnn_samples_kernels.hip), which narrows while it cuts: one statement of the arithmetic for both kernels.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime_api.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the device inlines at the end
#endif

namespace ethcnn {
namespace narrow {

constexpr int64_t kDefaultChunkBytes = 256LL << 20;  // narrow buffer of ethcnn_predict_luma16_device (as ethcnn_ldp_sequence's vectors)

inline int roundup16(int w) { return (w + 15) & ~15; }

// src: 2-byte aligned, pitch / frame stride in bytes and even; dst: 16-byte aligned, dst_pitch / dst_fstride multiples of 16,
// dst_pitch >= roundup16(width).  (The caller has checked all of that: ethcnn_narrow_luma_device.)
void launch_narrow(hipStream_t s, const uint8_t* src, int width, int height, long pitch, long fstride, int nframes, int shift,
                   uint8_t* dst, long dst_pitch, long dst_fstride, int cus);

// host form of the rule over n samples; nt: non-temporal stores (the destination is page-locked staging memory that the DMA engine
// reads next, never this CPU).  SSE2 body + scalar tail; scalar alone where the host ISA has no SSE2.
void narrow_row(const uint16_t* src, uint8_t* dst, size_t n, int shift, bool nt);

#if defined(__HIPCC__)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// two samples of a dword: min(s >> shift, 255) in each half (v_pk_lshrrev_b16, v_pk_min_u16)
__device__ __forceinline__ uint32_t narrow2(uint32_t d, int shift) {
    u16x2 v = __builtin_bit_cast(u16x2, d);
    v = v >> (u16x2)((unsigned short)shift);
    v = __builtin_elementwise_min(v, (u16x2)((unsigned short)255));
    return __builtin_bit_cast(uint32_t, v);
}

// the low bytes of the four narrowed samples in two dwords (lo: samples 0 and 1, hi: 2 and 3) as one output dword (v_perm_b32)
__device__ __forceinline__ uint32_t pack4(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x06040200u); }

// 16 samples in eight source dwords -> their 16 narrowed bytes
__device__ __forceinline__ uint4 narrow8(const uint32_t (&w)[8], int shift) {
    uint32_t s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = narrow2(w[i], shift);
    return make_uint4(pack4(s[0], s[1]), pack4(s[2], s[3]), pack4(s[4], s[5]), pack4(s[6], s[7]));
}
#endif

}  // namespace narrow
}  // namespace ethcnn
