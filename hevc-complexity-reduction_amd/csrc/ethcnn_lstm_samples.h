// ethcnn_lstm_samples.h -- shared between the ETH-LSTM sample-set kernels (ethcnn_lstm_samples_kernels.hip), their host side
// (ethcnn_lstm_samples.cpp) and the LSTM trainer's hand-off (ethcnn_lstm_train.cpp): include/ethcnn.h "ETH-LSTM sample sets".
//
// A build reads n 16516-byte LDP records that are resident in HBM (an inter sample set's buffer, or a copy uploaded piece by piece) and
// writes m x nslots 37264-byte samples, m = the heads of ethcnn_lstm_samples_plan.  Launches (all on the context's stream; no atomics,
// every output byte has one writer, the order of the samples is fixed by the host's scan):
//   k_lstm_headers         once: a lane per record, four aligned dword loads of the header -> {width | height << 16, i_frame} per record
//                          (8 n bytes); the host scans them (the loop ethcnn_lstm_samples_plan runs over host records) into the head
//                          rows and their per-frame strides, which go back as two int64 arrays [m]
//   per requested slot s, ascending:
//     per chunk of `chunk` records (a multiple of 32):
//       k_resi_repack      a block per CTU and trip: the slot's 4096 residual bytes start at byte 81 + 4113 s of a record, never on a
//                          word, so a lane loads the two 16-byte aligned words around its 16 bytes (the last word of the buffer by
//                          guarded dwords) and funnel-shifts them by the block-uniform offset; one dwordx4 store per lane into a picture
//                          2048 bytes (32 CTUs) across, CTU j of the chunk at row 64 (j / 32), column 64 (j % 32); the CTUs behind the
//                          chunk's last record, up to the end of their row, are zero-filled
//       ethcnn_resi_vectors_device on that picture -> rows [first record of the chunk ..) of the slot's vector array [n][448]
//     k_lstm_sample_gather a block per sample and trip (grid-stride), 9316 dwords each, four per lane in flight (loads before stores):
//                          dwords 0..15 the head's info bytes with byte 0 = 19; then for k = 0..19 the 465 floats of record
//                          head - k * stride: 17 bytes [QP | labels] of its slot converted to float, 448 floats of the vector array
// The vector array belongs to one slot at a time and is reused by the next.
//   k_lstm_qp0 / k_lstm_compact  the trainer's hand-off under a QP selection: the slot-0 QP float of every sample -> host, which lists
//                          the kept samples; sample j of the trainer's buffer = sample keep[j] of the set, dwordx4 copies
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "ethcnn_lstm_train.h"

namespace ethcnn {
namespace lstm_samples {

constexpr int kRecIn = train::kRecLdp;          // 16516
constexpr int kRecOut = lstm_train::kRecBytes;  // 37264
constexpr int kSteps = lstm_train::kSteps, kSlotFloats = lstm_train::kSlotFloats, kVec = lstm_train::kVec;
constexpr int kGroup = 17;                      // [QP | 16 labels] in front of a slot's residual
constexpr int kStride = 10;                     // LSTM_OVERLAP_STRIDE: a head every 10th frame, from frame 19 on
constexpr int kTileCols = 32, kPitch = kTileCols * 64;  // the repacked picture: 32 CTUs across
constexpr int kDefaultChunk = 8192;             // records per chunk: a 2048 x 16384 picture, 32 MB

struct Header {  // what k_lstm_headers keeps of a record
    uint32_t wh;       // width | height << 16
    uint32_t i_frame;
};

// the selection of include/ethcnn.h "ETH-LSTM sample sets" over n records whose headers `get(i)` returns, in record order
struct Plan {
    std::vector<int64_t> heads, strides;  // [m] record index of a head; records per frame of its own geometry
    int64_t skipped = 0;
};
template <typename Get>
inline void plan(int64_t n, Get get, Plan* p) {
    p->heads.clear();
    p->strides.clear();
    p->skipped = 0;
    for (int64_t r = 0; r < n; ++r) {
        const Header h = get(r);
        if (h.i_frame < (uint32_t)(kSteps - 1) || h.i_frame % kStride) continue;
        const int64_t per = (int64_t)((h.wh & 0xffff) / 64) * (int64_t)((h.wh >> 16) / 64);
        if (r - (kSteps - 1) * per < 0) {
            ++p->skipped;
            continue;
        }
        p->heads.push_back(r);
        p->strides.push_back(per);
    }
}
inline Header header_of(const uint8_t* rec) {
    Header h;
    h.wh = (uint32_t)rec[2] | (uint32_t)rec[3] << 8 | (uint32_t)rec[4] << 16 | (uint32_t)rec[5] << 24;
    h.i_frame = (uint32_t)rec[10] | (uint32_t)rec[11] << 8 | (uint32_t)rec[12] << 16 | (uint32_t)rec[13] << 24;
    return h;
}

// launchers (ethcnn_lstm_samples_kernels.hip); `rec` is 16-byte aligned and holds nrec records
void launch_headers(hipStream_t s, const uint8_t* rec, long nrec, Header* out, int cus);
void launch_repack(hipStream_t s, const uint8_t* rec, long nrec, long first, int n, int slot, uint8_t* picture, int cus);
void launch_sample_gather(hipStream_t s, const uint8_t* rec, const float* vec, const int64_t* heads, const int64_t* strides, long m, int slot,
                          uint8_t* out, int cus);
void launch_qp0(hipStream_t s, const uint8_t* samples, long n, float* qp0);
void launch_compact(hipStream_t s, const uint8_t* in, const int64_t* keep, long n, uint8_t* out, int cus);
void launch_copy16(hipStream_t s, const uint8_t* in, uint8_t* out, long nbytes, int cus);  // k_copy16: the float4 copy the rates are judged by

}  // namespace lstm_samples
}  // namespace ethcnn

struct ethcnn_ctx;
struct ethcnn_lstm_samples {
    ethcnn_ctx* c = nullptr;
    int slots[4] = {0, 1, 2, 3};  // ascending
    int nslots = 4;
    int chunk = 0;                // records per chunk
    uint64_t max_bytes = 0;
    int64_t count = 0, skipped = 0;
    uint8_t* data = nullptr;      // count x 37264 bytes in HBM once built
    bool built = false;
    std::string err;
};
