// ethcnn_lstm_seq.h -- config #5 offline: the ETH-LSTM recurrence of whole residual sequences (ethcnn_lstm_seq.hip).
// Launch list of one chunk of up to kLstmSeqBatchMax sequences, each with its own CTU count n and frames F (all on the context's
// main stream; a solo sequence is one row, a group K rows with the same n, F and first frame number):
//   front-end      launch_tile -> launch_trunk(resi) -> launch_fc1 over passes of whole frames, per sequence -> vec [F][n][448]
//                      (seq_front, ethcnn_ldp.cpp)
//   launch_lstm_seq_batch    ONE launch per run of frames that shares a start state, for all sequences: every block owns its 16-CTU
//                      column groups of one level of one sequence for all frames of the run; (c, h) never leave the CU; writes
//                      UNGATED probabilities [F][n][21] and the final (c, h) once
//   launch_lstm_seq_gates_batch   one block per (sequence, frame, 1024-CTU mini-batch): predicates by a block reduction over the
//                      ungated probabilities, then the zero-fill of ethcnn_lstm.hip's last block (the 0 > thr2 corner included)
// No block of either launch ever waits for another one.  The host side of the two launches is seq_launch (ethcnn_ctx.h).
#pragma once
#include <hip/hip_runtime.h>

namespace ethcnn {

// One sequence's part of a launch: the row the kernels read, and the only description of a sequence on the host.  Frames [0, F) of
// vec / probs; frame f carries i_frame = i_frame0 + f.  state_in: (c, h) [n][2][448] before frame 0, null = zeros; state_out: (c, h)
// after the last frame.  It may be the same buffer as the row's state_in: a block STORES only its own valid columns and its results
// depend only on its own columns of the input; the lanes of a ragged or surplus column group read row n - 1 (possibly after its owner
// has stored it), feed MFMA columns that are independent of all others, and are never stored.  No row's buffers may overlap another
// row's outputs.  Every row of a recurrence launch is one run: the caller (seq_launch) splits a sequence where the state is zeroed
// (i_frame <= 1), so a frame with i_frame <= 0 is a run of its own, and inside a run the state is always carried.
constexpr int kLstmSeqGroupMax = 8;   // members of a group (and of a replayed one, ethcnn_replay.cpp)
constexpr int kLstmSeqBatchMax = 32;  // rows of a launch
struct SeqBatchRow {
    const float* vec;       // [F][n][448]
    const float* state_in;  // [n][2][448] or null
    float* state_out;       // [n][2][448]
    const float* blob;      // the sequence's bundle image: payload + packed kernels
    float* probs;           // [F][n][21], ungated
    float efs0;             // lstm_seq_efs0(qp)
    alignas(8) int n;       // CTUs of a frame (a row is 64 bytes of the kernel arguments)
    int F, i_frame0;        // frames of this launch and the frame number of the first one
};
inline float lstm_seq_efs0(int qp) { return ((float)qp / 51.0f) * 0.18f; }  // net():283  qp / 51.0 * 0.18
// recurrence blocks of a sequence of n CTUs at level 16, 32, 64: G, ceil(G / 2), ceil(G / 4) with G = ceil(n / 16) column groups
inline void lstm_seq_blocks(int64_t n, int64_t out[3]) {
    const int64_t G = (n + 15) / 16;
    out[0] = G, out[1] = (G + 1) / 2, out[2] = (G + 3) / 4;
}
// rows in any order: the launch deals the blocks of a level to the rows with the most frames first (scheduling only)
void launch_lstm_seq_batch(const SeqBatchRow* rows, int k, hipStream_t s);
// the gate pass over the rows' probabilities [F][n][21] (reads probs, n and F of a row): row j under the pair thr1[j], thr2[j] (k
// entries each).  The scalar form gives every row the same pair.
void launch_lstm_seq_gates_batch(const SeqBatchRow* rows, int k, const float* thr1, const float* thr2, hipStream_t s);
void launch_lstm_seq_gates_batch(const SeqBatchRow* rows, int k, float thr1, float thr2, hipStream_t s);

// dependent v_mfma_f32_16x16x4_f32 links per frame of the wave that owns a hidden tile (its four gate chains are interleaved), and of
// the head waves, per level (64, 32, 16): what scripts/ldp_sequence_rate.py holds against the measured link latency
constexpr int kLstmSeqChainLinks[3] = {2 * 64 / 4, 2 * 128 / 4, 2 * 256 / 4};
constexpr int kLstmSeqHeadLinks[3] = {64 / 4 + 48 / 4, 128 / 4 + 96 / 4, 256 / 4 + 192 / 4};

}  // namespace ethcnn
