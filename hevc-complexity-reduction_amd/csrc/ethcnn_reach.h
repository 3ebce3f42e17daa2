// ethcnn_reach.h -- shared between the kernel of the threshold calibration on reached nodes (ethcnn_reach.hip) and its host side
// (ethcnn_reach.cpp): include/ethcnn.h "threshold calibration on reached nodes".
//
// k_reach_hist writes, per candidate, the histogram of the DECIDED NODES of the labelled CTUs in the calibrator's layout
// (ethcnn_calib.h: hist[level][truth][bin], 6150 words).  Lane = candidate with counters in registers, the shape of k_sim_eval, does
// not carry 6150 words, so here a block owns ONE candidate and a slice of the records, and a lane owns a record: the candidate's six
// thresholds and two gate thresholds are the same for the whole block, a lane reads its 64-byte record with four 16-byte loads, gets
// the masks of ethcnn_node_masks.h and adds one per decided node to the block's histogram in LDS (6150 x uint32 = 24,600 bytes, as
// k_calib_count holds); the non-zero words go to out[candidate] with 64-bit atomic adds at the end of the slice.  Integers only: the
// result does not depend on the grid.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "ethcnn_calib.h"

namespace ethcnn {
namespace reach {

constexpr int kHistWords = calib::kHistWords;  // ETHCNN_REACH_HIST_WORDS
constexpr int kMaxCand = 256;                  // ETHCNN_REACH_MAX_CAND
constexpr long kMaxSlice = 1L << 24;           // CTUs a block counts into 32-bit LDS words
// a word of the histogram is one (level, truth, bin): a CTU adds at most its 16 nodes of level 2 to it
static_assert(16 * kMaxSlice <= (1LL << 32) - 1, "a slice's adds fit a 32-bit LDS word");

// out[ncand][kHistWords] += the histograms of cand[ncand][6] (up_k[3], down_k[3]) over recs[0 .. n); out must be zeroed
void launch_hist(hipStream_t s, const unsigned* recs, const unsigned* m, long n, const int* cand, long ncand, int gate_order, unsigned long long* out,
                 int cus);

}  // namespace reach
}  // namespace ethcnn
