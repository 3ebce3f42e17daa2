// ethcnn_replay.h -- shared between the sample-set replay kernels (ethcnn_replay.hip) and their host side (ethcnn_replay.cpp):
// include/ethcnn.h "sample-set replay".
//
// A replay reads n 16516-byte Low-Delay-P records that are resident in HBM (an inter sample set's buffer, or a copy uploaded piece by
// piece), in any record order, and puts the residual pictures and label planes of a run back together for ethcnn_ldp_sequence_device.
// Launches (all on the context's stream; no atomics, every output byte has one writer):
//   k_replay_headers   once per open of a set: a lane per record, aligned dword loads only (words 0..4 of the header and the four words
//                      that hold a slot's QP byte) -> 20 bytes per record {w | h << 16, f, line | col << 16, seq, q0 | q1 << 8 | q2 << 16
//                      | q3 << 24}; the host builds the plan from them (the loop ethcnn_replay_plan runs over host records).  Records
//                      from host memory are planned there and this launch does not run.
//   per run and slot, per chunk of frames:
//     k_uncut_inter    a block per (frame, CTU) and trip, two CTUs in flight per block (loads of both before the stores of either):
//                      the record index comes from src[frame][ctu]; the slot's 4096 residual bytes start at byte 81 + 4113 s of the
//                      record, never on a word and at any of the 16 offsets from a 16-byte boundary, so a lane loads the two 16-byte
//                      aligned words around its 16 bytes (the word that would reach past the end of the buffer by guarded dwords) and
//                      funnel-shifts them by the block-uniform offset; one dwordx4 store per lane into the plane, whose pitch 64 C
//                      keeps every CTU row 16-byte aligned.  Lanes 0..3 also carry the 16 depth bytes (byte 65 + 4113 s on): two
//                      aligned dword loads, a funnel shift, one dword store into a row of the label plane.  An index outside
//                      [0, nrecords) writes zeros instead of reading.
//     ethcnn_ldp_sequence_device on the chunk's planes -> the run's probabilities; the (c, h) state goes from chunk to chunk by that
//                      call's resident-state rule
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "ethcnn_train.h"

namespace ethcnn {
namespace replay {

constexpr int kRec = train::kRecLdp;  // 16516
constexpr int kGroup = 17;            // [QP | 16 labels] in front of a slot's residual
constexpr int kMaxCtus = 1 << 20;     // CTUs per picture: 16-bit line and column counts, bounded so that products stay in range

struct Header {  // what k_replay_headers keeps of a record
    uint32_t wh;       // w | h << 16
    uint32_t f;        // frame number in encoding order
    uint32_t linecol;  // line | col << 16
    uint32_t seq;
    uint32_t qps;      // q0 | q1 << 8 | q2 << 16 | q3 << 24
};

inline Header header_of(const uint8_t* r) {
    Header h;
    h.wh = (uint32_t)r[2] | (uint32_t)r[3] << 8 | (uint32_t)r[4] << 16 | (uint32_t)r[5] << 24;
    h.f = (uint32_t)r[10] | (uint32_t)r[11] << 8 | (uint32_t)r[12] << 16 | (uint32_t)r[13] << 24;
    h.linecol = (uint32_t)r[14] | (uint32_t)r[15] << 8 | (uint32_t)r[16] << 16 | (uint32_t)r[17] << 24;
    h.seq = (uint32_t)r[18] | (uint32_t)r[19] << 8;
    h.qps = 0;
    for (int s = 0; s < 4; ++s) h.qps |= (uint32_t)r[train::kSlotBase + train::kSlotBytes * s] << (8 * s);
    return h;
}

struct Run {
    int seq, w, h, R, C;
    uint32_t f0;
    int64_t F, nctu;
    int qp[4];
    int64_t src_at;  // first entry of the run in Plan::src
};
struct Plan {
    std::vector<Run> runs;
    std::vector<int64_t> src;  // run after run, [F][nctu] record indices
};
// the plan of include/ethcnn.h "sample-set replay" over n headers; false: *why names the record and the rule (ethcnn_replay.cpp)
bool plan(const Header* h, int64_t n, Plan* out, std::string* why);

// launchers (ethcnn_replay.hip); `rec` is 4-byte aligned and holds nrec records
void launch_headers(hipStream_t s, const uint8_t* rec, long nrec, Header* out, int cus);
void launch_uncut(hipStream_t s, const uint8_t* rec, long nrec, const int64_t* src, long nframes, int R, int C, int slot, uint8_t* resi,
                  uint8_t* labels, int cus);

}  // namespace replay
}  // namespace ethcnn

struct ethcnn_ctx;
struct ethcnn_replay {
    ethcnn_ctx* c = nullptr;
    uint64_t max_bytes = 0;
    int chunk = 0;                  // frames per chunk, 0 = default
    const uint8_t* rec = nullptr;   // the records in HBM: a set's buffer, or `own`
    uint8_t* own = nullptr;         // the uploaded copy of host records
    int64_t nrec = 0;
    ethcnn::replay::Plan plan;
    // working buffers, grown on demand and kept until the next open / destroy
    uint8_t* d_resi = nullptr;      // one chunk's residual planes
    size_t resi_cap = 0;
    int64_t* d_src = nullptr;       // the src table of the run last replayed
    size_t src_cap = 0;
    int src_run = -1;               // the run whose table d_src holds
    float* d_probs = nullptr;       // a run's probabilities, when the caller brings no buffer
    size_t probs_cap = 0;
    uint8_t* d_labels = nullptr;    // a run's label planes, when the caller brings no buffer
    size_t labels_cap = 0;
    float* d_zero = nullptr;        // a zero (c, h) state for runs that start behind frame 1
    size_t zero_cap = 0;
    std::string err;
};
