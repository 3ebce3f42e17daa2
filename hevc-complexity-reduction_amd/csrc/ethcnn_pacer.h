// ethcnn_pacer.h -- shared between the kernels of the online search budget (ethcnn_pacer.hip) and their host side (ethcnn_pacer.cpp):
// include/ethcnn.h "search budget, online".
//
// A frame is two launches on the context's stream and no memset:
//   k_pacer_frame  probs float [per][21] (raster, as the predictors write them) -> the frame's records in the scratch (ethcnn_sim.h: 64
//                  bytes a CTU, truth = 0, sub-batch = 0), checked uint32 [rungs][4] (the full search is the last rung), the choice, the
//                  carry, the frame count, the one-row threshold table and the result.
//     Launch: blocks of 256 lanes; block -> (slice, rung block), rung block fastest.  A slice is at most kSliceCtus CTUs of the frame, a
//     rung block 4 waves x 64 rungs.  Every block packs ITS slice into LDS (a lane is a CTU; the arithmetic is k_sim_pack's, restated);
//     rung block 0 also stores the records to the scratch.  After the barrier a lane is a rung: the wave walks the slice's records out of
//     LDS (every lane reads the same address: a broadcast), runs sim::compare_bins / sim::descend and adds its four 32-bit counters to
//     the table with integer atomics.  Then the block draws a ticket (agent-scope release before, acquire after); no block waits for
//     another.  The block with the last ticket reads the table with agent-scope atomic loads, makes the choice of ethcnn_budget_choose
//     in unsigned __int128 (a block-wide minimum: no monotone ladder is assumed), updates the state and zeroes table and ticket again.
//   k_budget_bake  (ethcnn_budget.hip, unchanged) on the scratch records with per = nctu, ctu0 = 0 and the one-row table.
// The host form adds k_pacer_done, one lane that stores the context's completion word behind the bake.
//
// State words in HBM (unsigned [kStateWords]), zero at create and after reset; between frames ticket and table are zero by construction:
//   [0] ticket   [2..3] frames paced (uint64)   [4..7] carry (128 bits, low word first)   [8..13] the picked rung's up_k[3], down_k[3]
#pragma once
#include <cstdint>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/ethcnn.h"

struct ethcnn_ctx;

namespace ethcnn {
namespace pacer {

constexpr int kSliceCtus = 64;  // CTUs of a slice at most: 4 KB of records in LDS, and the length of a wave's walk
constexpr int kStateWords = 16;
constexpr int kStateTicket = 0, kStateFrame = 2, kStateCarry = 4, kStateThr = 8;

struct FrameArgs {
    const float* probs;      // [per][21]
    int width, height, ctus_w;
    int per;                 // CTUs of the frame
    const int* thr;          // [rungs][6]
    int rungs;               // K + 1
    unsigned* checked;       // [rungs][4]
    unsigned* state;         // [kStateWords]
    unsigned* recs;          // scratch [per][16]
    unsigned long long weight[4];
    unsigned budget_ppm;
    int carry_mode;          // 1: ETHCNN_BUDGET_CARRY
    ethcnn_pacer_result* d_result;  // may be NULL
    ethcnn_pacer_result* h_result;  // the page-locked slot
};

// blocks of a frame of `per` CTUs under `rungs` rungs (slices x rung blocks)
long frame_blocks(long per, int rungs);
void launch_frame(hipStream_t s, const FrameArgs& a);
void launch_done(hipStream_t s, unsigned* h_done, unsigned seq);

// ---- host side, shared with the pacer set (ethcnn_pacer_set.cpp); definitions: ethcnn_pacer.cpp
// the rules of the ladder, the weights, the budget and the mode; c may be NULL (the message then goes where ethcnn_last_error(NULL) reads)
int check_rules(ethcnn_ctx* c, const ethcnn_sim_thr* ladder, int64_t K, const uint64_t* weight, uint32_t budget_ppm, int mode);
// W, H and the cost bound of a frame under `weight`; *per = its CTUs
int check_frame(ethcnn_ctx* c, const uint64_t weight[4], int width, int height, int64_t* per);
// a device buffer of at least `want` units of bytes_each; growing waits for the work in flight on the context's stream
int grow(ethcnn_ctx* c, void** buf, int64_t* cap, int64_t want, int64_t bytes_each, const char* what);
// the ladder (NULL: the default one) with the full search appended, as int32 rows up_k[3], down_k[3]
std::vector<int> ladder_rows(const ethcnn_sim_thr* ladder, int64_t K);

}  // namespace pacer
}  // namespace ethcnn
