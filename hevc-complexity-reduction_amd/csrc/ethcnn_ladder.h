// ethcnn_ladder.h -- shared between the kernel of the ladder search (ethcnn_ladder.hip) and its host side (ethcnn_ladder.cpp):
// include/ethcnn.h "search budget: building a ladder".
//
// A step is ONE launch of k_ladder_step on the context's stream and no memset:
//   A lane is a candidate (c, v): coordinate c in the sweep order down0, up0, down1, up1, down2, up2 and value v = m * grid.  It is made
//   in the kernel from the current thresholds in the state block, so nothing is uploaded per step.  A coordinate owns
//   ceil(slots / 64) candidate waves (slots = 1025 / grid + 1, of which m = 0 .. 1024 / grid are values), so c is the same for a whole
//   wave and five of a lane's six thresholds are wave-uniform.  wave -> (slice, candidate wave), candidate wave fastest; a slice is a run
//   of CTUs of at most sim::kMaxSlice, so the 32-bit lane counters are exact.  The record address is wave-uniform as in k_sim_eval.  A
//   lane keeps checked[0..3] and the bad CTUs (gates none) and adds them to table[c][m][0..4] with agent-scope integer atomics.
//   Then the block draws a ticket as k_pacer_frame does (agent-scope release before, acquire after; no block waits for another).  The
//   block with the last ticket reads the table with agent-scope atomic loads, finds per coordinate the nearest value with a lower cost
//   (a block-wide minimum), applies the cap, makes the six-way choice in __int128, appends the rung, updates the state and zeroes table
//   and ticket again.  A launch that finds the done flag set exits at once.
//
// State words in HBM (unsigned long long [kStateWords]); between steps ticket and table are zero by construction:
//   [0] ticket   [1] done   [2] rungs so far   [3..5] up_k   [6..8] down_k (as int64)   [9] cost C   [10] bad CTUs B
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

struct ethcnn_ladder_rung;

namespace ethcnn {
namespace ladder {

constexpr int kStateWords = 16;
constexpr int kStateTicket = 0, kStateDone = 1, kStateRungs = 2, kStateUp = 3, kStateDown = 6, kStateCost = 9, kStateBad = 10;
constexpr int kTableFields = 5;  // checked[0..3], bad CTUs
constexpr int kBatch = 64;       // steps enqueued between two looks at the state

// slots of a coordinate in the table / values of a coordinate
inline int slots_of(int grid) { return 1025 / grid + 1; }
inline int values_of(int grid) { return 1024 / grid + 1; }

struct StepArgs {
    const unsigned* recs;        // the simulator's records [n][16]
    long n;
    unsigned long long* state;   // [kStateWords]
    unsigned long long* table;   // [6][slots][kTableFields]
    ethcnn_ladder_rung* rungs;   // [max_rungs]
    unsigned long long weight[4];
    unsigned long long cap;      // max_bad_ppm * labelled CTUs: a move needs bad * 10^6 <= cap
    int grid, slots, values;
    int max_rungs;
};

void launch_step(hipStream_t s, const StepArgs& a, int cus);

}  // namespace ladder
}  // namespace ethcnn
