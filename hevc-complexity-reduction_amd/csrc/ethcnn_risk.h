// ethcnn_risk.h -- shared between the kernels of the expected wrong decisions (ethcnn_risk.hip) and their host side
// (ethcnn_risk.cpp): include/ethcnn.h "partition-search simulation: expected wrong decisions".
//
// The reliability table lies in HBM as unsigned [3][1025] (level, bin), every value in 0..kOne.  Both kernels read it at addresses
// that are the same for a whole wave (the bins come from the record, whose address is wave-uniform), so the 21 values of a record are
// fetched once per wave and record, not per lane.
//
// k_sim_risk has the shape of k_sim_eval (ethcnn_sim.hip): a lane is a candidate, a wave owns 64 candidates and a slice of the records.
// Per lane and record two masks (CURRENT ONLY and SPLIT ONLY among the decided nodes, from ethcnn_node_masks.h) pick which of the 21
// values, or of their complements to kOne, go into six 32-bit sums (a level's sum stays below 16 * 2^20 = 2^24); these are added to
// the lane's six 64-bit accumulators once per record, and those to out[candidate][6] with 64-bit atomic adds at the end of the slice.
//
// k_ladder_step_risk is the step of ethcnn_ladder_step.h with a table row of ten words: checked[0..3], exp_wrong_split[3],
// exp_wrong_stop[3].  The state word kStateBad holds the risk of the current rung.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

struct ethcnn_ladder_rung_risk;

namespace ethcnn {
namespace risk {

constexpr unsigned kOne = 1u << 20;  // ETHCNN_RISK_ONE
constexpr int kBins = 1025;
constexpr int kRelWords = 3 * kBins;
constexpr int kFields = 6;           // uint64 words of an ethcnn_sim_risk: exp_wrong_split[3], exp_wrong_stop[3]
constexpr int kTableFields = 4 + kFields;

// out[ncand][kFields] += the expected wrong decisions of cand[ncand][6] (up_k[3], down_k[3]) over recs[0 .. n); out must be zeroed
void launch_risk(hipStream_t s, const unsigned* recs, long n, const int* cand, long ncand, const unsigned* rel, unsigned long long* out, int cus);

struct StepArgs {
    const unsigned* recs;        // the simulator's records [n][16]
    long n;
    unsigned long long* state;   // [ladder::kStateWords]
    unsigned long long* table;   // [6][slots][kTableFields]
    ethcnn_ladder_rung_risk* rungs;  // [max_rungs]
    const unsigned* rel;         // [3][1025]
    unsigned long long weight[4];
    unsigned long long cap_lo, cap_hi;  // max_risk_ppm * counted CTUs * kOne in 128 bits: a move needs risk * 10^6 <= cap
    int grid, slots, values;
    int max_rungs;
};

void launch_step(hipStream_t s, const StepArgs& a, int cus);

}  // namespace risk
}  // namespace ethcnn
