// ethcnn_lstm_train.h -- shared between the ETH-LSTM training kernels (ethcnn_lstm_train_kernels.hip) and their host side
// (ethcnn_lstm_train.cpp: a trainer's state; ethcnn_lstm_train_group.cpp: the step engine behind the solo and the group entry
// points).  Graph: ETH-LSTM_Training_LDP/net_CTU64.py:85-276, samples: input_data.py:88-147, optimiser:
// train_LSTM_CTU64.py:42-52.
//
// A sample is 37264 bytes: 64 info bytes, then 20 time slots of 465 float32 [qp | 16 depth labels | 448-vector]
// (input_data.py:94-108).  Slot 0 is the current frame, slot k frame i - k.  At batch B a step works on R = 20 B rows,
// row r = 20 b + p for slot p of batch sample b (the order net_CTU64.py:207-216 flattens labels and predictions in).
// Three independent LSTMCells (hidden 64 / 128 / 256 on vector columns [0,64) / [64,192) / [192,448); forget_bias 1, cell_clip 5,
// gate order i, j, f, o) consume slot 19 first and slot 0 last (cell_inputs.reverse(), :109); the prediction list is reversed
// back (:137), so the prediction of row (b, p) is the one computed when slot p was the input.  The external features are NOT
// reversed: unrolled step ts (input slot 19 - ts) is given qp_list[ts] and the GOP one-hot of slot ts (:125), so row (b, p) sees
// the QP and the GOP position of slot 19 - p.  This is how the shipped models were trained; it is transcribed, not corrected.
//
// There is ONE step path.  It trains K >= 1 models ("members") of one batch size at once; a solo trainer is the case K = 1.  One
// training step is 10 launches on the context's stream, each over all K members (grids: "the member table" below):
//   1 k_lstm_group_gather     one block per row: draw / read the sample index, copy the 448-vector and the 16 labels, form the five
//                             external features [qp / 51 (* qp_scale) | one-hot(i_frame_in_GOP)] of slot 19 - p
//   2 k_group_gemm            input projections of all 20 slots and all three cells: X[R, H] x kernel[0:H, :] -> Z [R, 4H], one
//                             grouped launch of the CNN trainer's MFMA 32x32x2 GEMM (ethcnn_train_kernels.hip), three descriptors
//   3 k_lstm_group_fwd        recurrence: a block owns 16 batch samples of one cell and walks the 20 steps, h_prev x kernel[H:2H, :]
//                             as v_mfma_f32_16x16x4_f32 chains (a wave owns hidden-unit tiles and their four gates, so the gate math
//                             needs no exchange; h goes round through LDS); keeps gates, c before and after the clip, and h per row
//   4 k_lstm_group_heads_fwd  one block per row: dropout on the cell output (keep 0.5; the carried h is not dropped), fc2 +
//                             leaky-ReLU + dropout (keep 0.8), fc3 + sigmoid of the three cells
//   5 k_group_loss            one block per member: batch-global counts over all R rows, loss / accuracy lists, dL/dlogit (the CNN
//                             trainer's kernel: net_CTU64.py:160-176,220-233,263-271 are the CNN graph's labels, balanced loss and
//                             accuracy over R rows)
//   6 k_lstm_group_heads_bwd  one block per row: dlogit -> d fc2 -> d(cell output)
//   7 k_lstm_group_bwd        recurrence backwards (slot 0 first), same ownership as 3: d gates per row, dh carried through
//                             kernel[H:2H, :]^T (MFMA 16x16x4), dc through the forget gate; zero where c was clipped
//   8 k_group_gemm            every weight gradient as one grouped GEMM with K = R: [x | h_prev | 1]^T x dZ for the three kernels and
//                             biases, [h (dropped) | ef | 1]^T x dZ2 and [h2 (dropped) | ef | 1]^T x dZ3 for the heads; blob layout
//   9 k_lstm_group_norm       partial sums of squares of the 760078 gradient floats: 512 blocks, each a fixed range and a fixed order
//  10 k_lstm_group_update     every block sums the 512 partials in index order -> global norm, clip_by_global_norm's factor, momentum
//                             update
// Evaluation runs launches 1-4 on chunks of samples (no dropout) into one probability / label array and then ONE launch 5 over all
// of its rows.  Determinism: no atomics; every sum has one owner and a fixed order.
#pragma once
#include <cstdint>

#include "ethcnn_train.h"

namespace ethcnn {
namespace lstm_train {

using train::draw;
using train::mix64;

constexpr int kSteps = 20;                  // LSTM_MAX_LENGTH = LSTM_READ_LENGTH = LSTM_OUTPUT_LENGTH (config.py:15-18)
constexpr int kSlotFloats = 465;            // [qp | 16 labels | 448 vector]
constexpr int kRecBytes = 64 + 4 * kSlotFloats * kSteps;  // 37264
constexpr int kVec = 448, kOut = 21, kFc2 = 336, kEf = 5;
constexpr int kLdH1 = 466, kLdH2 = 354;     // per cell [activations | qp | one-hot 4 | 1]
constexpr int kNormBlocks = 512;
enum { kStreamLstmIndex = 4, kStreamLstmDropout = 5, kStreamLstmInit = 6 };

// blob float offsets (kLstmTensors), cells in head order 64, 32, 16
struct LstmOffsets {
    int kern[3], bias[3], w2[3], b2[3], w3[3], b3[3];
};

struct LstmBufs {
    float* X;      // [R][448]
    float* lab;    // [R][16]
    float* E;      // [R][5]
    float* Z[3];   // [R][4H]: input projections, overwritten by the activated gates i, j, f, o
    float* Cpre;   // [R][448] c before the clip
    float* C;      // [R][448] c after the clip
    float* Hout;   // [R][448] h (not dropped)
    float* HP[3];  // [R][H + 1]: h of the previous step (slot p + 1; zeros at slot 19) and a ones column
    float *M1, *H1, *A2, *M2, *H2, *P;  // [R][448], [R][466], [R][336], [R][336], [R][354], [R][21]
    float *dZ3, *dZ2, *dH;               // [R][21], [R][336], [R][448]
    float* dZ[3];                        // [R][4H]
};

// ---- the member table (include/ethcnn.h "ETH-LSTM training" and "ETH-LSTM training, several models at once"): K >= 1 independent
// LSTM trainers of one batch size in every launch of a step.  Launch i of the 10 above covers all K members:
//   gather / heads forward / heads backward     grid (20 B, K): block (r, m) is row r of member m
//   GEMMs (projections, weight gradients)       the CNN trainer's k_group_gemm: K x T blocks, T = the tiles of one member's descriptors
//   recurrences                                 grid (ceil(B / 16), 3, K): block (s, cell, m)
//   loss                                        the CNN trainer's k_group_loss: K blocks, block m owns member m's counts over 20 B rows
//   norm / update                               grid (512, K) / (1024, K): gridDim.x, hence chunk and stride, do not depend on K
// The member is the grid's last dimension, no sum crosses members and nothing is atomic.  There is no other path, so member m
// computes the same bits whatever K and m are, a solo trainer (K = 1) included.
// The members share the two sample sets: one copy each, and per member and set the list of the records its QP selection keeps, in
// file order (keep NULL: all).  A member's sample index i is its i-th kept record, and its index draw is over nkept.  A solo trainer
// holds only the records it keeps (its uploads compact them), so its keep lists are NULL.
// The table lives in device memory and changes only with the sample sets; the host marks it stale then and uploads it again before
// the next step, after waiting for the steps in flight.  What changes per launch goes by value (LstmGroupStep, and train::GroupRates
// for the K learning rates of the step).  An evaluation works on tables of its own (one per piece), never on the step table.
struct LstmMember {
    LstmBufs u;
    float *W, *acc, *grad;  // blob layout
    double* part;           // [kNormBlocks]
    float* stats;           // [8]
    const int32_t* idx_in;  // explicit batch / evaluation samples (ignored when LstmGroupStep.drawn)
    int32_t* idx;           // the batch's sample indices, as drawn or read
    const int64_t* keep[2];  // per set: the kept records (NULL: every record)
    long nkept[2];
    uint64_t seed;
    float qp_scale;
    int dropout;
    float momentum, clip;
};
struct LstmGroupStep {
    const uint8_t* data;  // the shared records of `set`
    uint64_t step;
    int set;
    int drawn;  // 1: indices drawn on the device
};

// launchers (ethcnn_lstm_train_kernels.hip)
void launch_check_list(hipStream_t s, const uint8_t* data, const int64_t* list, long n, uint8_t* bad, int nblocks);
void launch_group_gather(hipStream_t s, int nb, int k, const LstmMember* tab, const LstmGroupStep& g);
void launch_group_fwd(hipStream_t s, int nb, int k, const LstmMember* tab, const LstmOffsets& o);
void launch_group_heads_fwd(hipStream_t s, int nb, int k, const LstmMember* tab, const LstmOffsets& o, uint64_t step, int train);
void launch_group_heads_bwd(hipStream_t s, int nb, int k, const LstmMember* tab, const LstmOffsets& o);
void launch_group_bwd(hipStream_t s, int nb, int k, const LstmMember* tab, const LstmOffsets& o);
void launch_group_norm_update(hipStream_t s, int k, const LstmMember* tab, const train::GroupRates& r, long n);

}  // namespace lstm_train
}  // namespace ethcnn
