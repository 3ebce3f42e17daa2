// ethcnn_samples.h -- shared between the sample-set kernels (ethcnn_samples_kernels.hip), their host side (ethcnn_samples.cpp) and the
// trainer's hand-off (ethcnn_train.cpp): include/ethcnn.h "sample sets".
//
// Launches (all on the context's stream; no atomics, every output byte has one writer):
//   k_cut_ai<A>     a grid-stride loop over records, two records in flight per block: 256 lanes x 16 bytes = the 64 x 64 luma tile
//                   (A = 16: one dwordx4 load per lane; A = 4 / 1: dword / byte loads for bases and pitches that are not 16-byte
//                   aligned), one dwordx4 store per lane into the record; lanes 0..55 also write the 896-byte tail (64 fill bytes
//                   and 52 label rows, 255 where the QP is not in the list) as dwordx4 stores
//   k_cut_ai16<A>   k_cut_ai over 16-bit luma (CutArgs::deep): a lane owns the same 16 samples, now 32 source bytes (A = 16: two
//                   dwordx4 loads; A = 4: eight dword loads; A = 2: sixteen 16-bit loads), narrows them by the rule of include/ethcnn.h
//                   (the device inlines of ethcnn_narrow.h: a packed shift and a packed minimum per source dword, a byte permute per
//                   output dword) and stores the same dwordx4; tail, loop, block count and record stores as k_cut_ai
//   k_cut_inter<A>  one record per block and trip: the four residual tiles go to LDS with the same wide loads (16 KB, aligned), the
//                   header and the four [QP | 16 labels] groups to a 132-byte LDS area; the record leaves as 4129 coalesced dwords,
//                   each funnel-shifted out of two aligned LDS words (a slot's residual starts at byte 81 + 4113 s, never on a word)
//   k_gather<V>     out record j = set record perm(first + j) (or first + j), dwordx4 (All-Intra) or dword (inter) copies
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "ethcnn_train.h"

namespace ethcnn {
namespace samples {

constexpr int kKindAi = 0, kKindInter = 1;  // ETHCNN_SAMPLES_AI / _INTER
constexpr int kStreamPermute = 7;           // draw() stream of the record permutation (1..3: ethcnn_train.h, 4..6: ETH-LSTM trainer)
constexpr int kHeaderBytes = 64, kGroupBytes = 17;  // inter record: header, then per slot [QP | 16 labels] in front of 4096 residual bytes

// The permutation of [0, count) fixed by (seed, count), written out in include/ethcnn.h: a four-round Feistel network over 2 * half
// bits (the smallest even width that holds count - 1, at least 2), cycle-walked into [0, count).
__host__ __device__ inline uint64_t perm(uint64_t seed, uint64_t count, uint64_t j) {
    int half = 1;
    while (half < 32 && (1ull << (2 * half)) < count) ++half;
    const uint64_t mask = (1ull << half) - 1;
    uint64_t x = j;
    do {
        uint64_t l = x >> half, r = x & mask;
        for (uint64_t round = 0; round < 4; ++round) {
            const uint64_t f = train::draw(seed, kStreamPermute, count, r, round) & mask;
            const uint64_t nl = r;
            r = l ^ f;
            l = nl;
        }
        x = l << half | r;
    } while (x >= count);
    return x;
}

// one launch: `nrec` records = frames x whole CTUs of a picture, record r = (frame r / (nl nc), CTU line, CTU column) in raster order
struct CutArgs {
    const uint8_t* luma[4];    // All-Intra: [0] only; inter: the residual plane of slot s
    long pitch[4], fstride[4];  // in bytes
    const uint8_t* label[52];  // All-Intra: by QP (NULL: that row stays 255); inter: by slot.  (h / 16) x lw bytes per frame
    long label_fstride;
    int label_al4;             // label bases and lw are multiples of 4: a CTU's four label runs are dword loads
    int qps[4];                // inter: the slot QP bytes
    int width, height, nl, nc, lw;
    long nrec;
    int frame0, seq;           // inter header: frame number of the first frame (then + 1 per frame), sequence number
    uint8_t* out;              // first record written
    int deep, shift;           // All-Intra: luma[0] holds 16-bit samples, a record takes min(s >> shift, 255) (k_cut_ai16)
};

// align: what the luma bases, pitches and frame strides are all multiples of (16, 4, or less)
void launch_cut(hipStream_t s, int kind, const CutArgs& a, int align, int cus);
void launch_gather(hipStream_t s, int kind, const uint8_t* in, uint8_t* out, long first, long n, long count, uint64_t seed, int permuted,
                   int cus);

}  // namespace samples
}  // namespace ethcnn

struct ethcnn_ctx;
struct ethcnn_samples {
    ethcnn_ctx* c = nullptr;  // NULL: validation and counting only
    int kind = 0, order = 0, nqps = 0;
    int qps[52] = {0};
    uint64_t max_bytes = 0;
    int bit_depth = 8, chroma = 420;  // source format of the sequences added next (ethcnn_samples_set_source_format)
    struct Seq {
        int w, h;
        int bit_depth, chroma;
        int64_t luma_bytes, frame_bytes;  // of one frame of the YUV (ethcnn_source_frame_bytes)
        int64_t frames, first_rec, nrec;
        std::vector<std::string> yuv, labels;
    };
    std::vector<Seq> seqs;
    int64_t count = 0;
    uint8_t* data = nullptr;  // count x record_bytes in HBM once built
    bool built = false;
    std::string err;
    int record_bytes() const { return kind == ethcnn::samples::kKindAi ? ethcnn::train::kRec : ethcnn::train::kRecLdp; }
};
