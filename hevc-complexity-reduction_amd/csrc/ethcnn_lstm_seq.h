// ethcnn_lstm_seq.h -- config #5 offline: the ETH-LSTM recurrence of a whole residual sequence (ethcnn_lstm_seq.hip).
// Launch list of one chunk of F frames of n CTUs (all on the context's main stream):
//   front-end      launch_tile -> launch_trunk(resi) -> launch_fc1 over passes of whole frames  -> vec [F][n][448]   (ethcnn_ldp.cpp)
//   launch_lstm_seq    ONE launch per run of frames that shares a start state: every block owns its 16-CTU column groups of one
//                      level for all frames of the run; (c, h) never leave the CU; writes UNGATED probabilities [F][n][21] and the
//                      final (c, h) once
//   launch_lstm_seq_gates   one block per (frame, 1024-CTU mini-batch): predicates by a block reduction over the ungated
//                      probabilities, then the zero-fill of ethcnn_lstm.hip's last block (the 0 > thr2 corner included)
// No block of either launch ever waits for another one.
#pragma once
#include <hip/hip_runtime.h>

namespace ethcnn {

// frames [0, nframes) of vec / probs; frame f carries i_frame = i_frame0 + f.  d_state_in: (c, h) [n][2][448] before frame 0, null =
// zeros; d_state_out: (c, h) after the last frame.  It may be the same buffer as d_state_in: a block STORES only its own valid
// columns and its results depend only on its own columns of the input; the lanes of a ragged or surplus column group read row n - 1
// (possibly after its owner has stored it), feed MFMA columns that are independent of all others, and are never stored.
// The caller splits a sequence where the state is zeroed (i_frame <= 1): inside a run the state is always carried.
void launch_lstm_seq(const float* d_vec, const float* d_state_in, float* d_state_out, const float* d_lstm_blob, int n, int nframes,
                     int qp, int i_frame0, float* d_probs, hipStream_t s);
void launch_lstm_seq_gates(float* d_probs, int n, int nframes, float thr1, float thr2, hipStream_t s);

// ---- group form (ethcnn_ldp_group.cpp): K <= kLstmSeqGroupMax independent sequences of one geometry, one run of frames and one
// i_frame0 share the two launches.  A member brings what differs: its vectors, states, bundle image, probabilities and QP feature
// (lstm_seq_efs0(qp): the expression of launch_lstm_seq).  The blocks of member m run the body of launch_lstm_seq on m's pointers, so
// every member's result is that launch's, bit for bit; the rule for state_in == state_out above holds per member, and no member's
// buffers may overlap another member's outputs.  launch_lstm_seq_gates_group: the gate pass over every member's probabilities.
constexpr int kLstmSeqGroupMax = 8;
struct SeqMember {
    const float* vec;       // [F][n][448]
    const float* state_in;  // [n][2][448] or null
    float* state_out;       // [n][2][448]
    const float* blob;      // the member's bundle image: payload + packed kernels
    float* probs;           // [F][n][21]
    float efs0;
};
inline float lstm_seq_efs0(int qp) { return ((float)qp / 51.0f) * 0.18f; }
void launch_lstm_seq_group(const SeqMember* members, int k, int n, int nframes, int i_frame0, hipStream_t s);
void launch_lstm_seq_gates_group(float* const* d_probs, int k, int n, int nframes, float thr1, float thr2, hipStream_t s);

// dependent v_mfma_f32_16x16x4_f32 links per frame of the wave that owns a hidden tile (its four gate chains are interleaved), and of
// the head waves, per level (64, 32, 16): what scripts/ldp_sequence_rate.py holds against the measured link latency
constexpr int kLstmSeqChainLinks[3] = {2 * 64 / 4, 2 * 128 / 4, 2 * 256 / 4};
constexpr int kLstmSeqHeadLinks[3] = {64 / 4 + 48 / 4, 128 / 4 + 96 / 4, 256 / 4 + 192 / 4};

}  // namespace ethcnn
