// ethcnn_pacer_set.h -- shared between the kernels of the pacer set (ethcnn_pacer_set.hip) and their host side (ethcnn_pacer_set.cpp):
// include/ethcnn.h "search budget, online: several sequences".
//
// A call over n frames, each of another slot, is two launches on the context's stream and no memset:
//   k_pacer_table       k_pacer_frame (ethcnn_pacer.h) over a TABLE of frames.  The table is a kernel argument; segment j owns the blocks
//                       [first_block, first_block + nblocks), nblocks = slices x rung blocks with the rung block fastest, and a block
//                       finds its segment by a scalar walk over first_block (the block index is uniform).  From there on the block does
//                       for its segment's frame what k_pacer_frame does: pack its slice through LDS, rung block 0 stores the records at
//                       recs + rec0, a lane is a rung and the wave walks the records by LDS broadcast, the counters go to the table of
//                       the segment's SLOT, the ticket is drawn from that slot's state word, and the block that draws ticket nblocks - 1
//                       of the SEGMENT makes that slot's choice, updates its carry and frame count, writes its one-row threshold table
//                       and its results and zeroes its table and ticket.  No block waits for another.
//   k_pacer_bake_table  k_budget_bake (ethcnn_budget.h) over the same table: a block is 256 consecutive CTUs of ONE segment, a lane a CTU,
//                       the thresholds are the row the slot's choice left in its state words.
// Per slot, in HBM: the state words of ethcnn_pacer.h (unsigned [nslots][kStateWords]) and checked uint32 [nslots][rungs][4], both zero
// between calls but for carry, frame count and the last picked row.
//
// POLICIES.  A set holds 1..kPacerSetMaxPolicies policies {ladder, weights, budget, mode}; every slot is bound to one of them.  In HBM,
// written once at create: all ladders concatenated in one int [sum of rungs][6], each with its full-search row appended, and one
// PolicyRec per policy.  A segment names its policy and its own rung_blocks = ceil(rungs of that policy / 256), so one launch mixes
// segments of 1 and of 17 rung blocks: nblocks = slices x rung_blocks is the ticket target of THAT segment, the lane -> rung mapping, the
// dead-lane clamp (rungs - 1 of that policy's rows), the choice loop, the weights, the allowance, the carry rule and the zeroing all
// come from the policy record, which the block reads once (the index is block-uniform: scalar loads).  A set of ONE policy runs the
// same kernel source in a second form that takes the record from the kernel argument instead, as before there were policies.  checked is
// [nslots][stride][4] with stride = the most rungs of any policy, so that binding a slot to another policy reallocates nothing.  A set
// made by ethcnn_pacer_set_create is a set of one policy bound to every slot.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "ethcnn_pacer.h"
#include "ethcnn_pacer_set_plan.h"

namespace ethcnn {
namespace pacer {

constexpr int kPacerSetMaxPolicies = 32;  // ETHCNN_PACER_SET_MAX_POLICIES

struct TableSeg {
    const float* probs;             // [per][21]
    ethcnn_pacer_result* d_result;  // may be NULL
    long rec0;                      // its first record in the scratch
    int width, height, ctus_w;
    int per;                        // CTUs of the frame
    int first_block, nblocks;       // of k_pacer_table
    int slice_len;                  // CTUs of a slice (the same under every rung block)
    int slot;
    int policy;                     // of the slot when the call was made
    int rung_blocks;                // ceil(rungs of that policy / 256)
};

struct PolicyRec {                  // 48 bytes
    int first_row;                  // of its ladder in thr
    int rungs;                      // K + 1
    int carry_mode;                 // 1: ETHCNN_BUDGET_CARRY
    unsigned budget_ppm;
    unsigned long long weight[4];
};

struct FrameTable {
    TableSeg seg[kPacerSetMax];
    int nseg;
    int stride;                     // rows of a slot's table: the most rungs of any policy
    const PolicyRec* policy;        // [npolicies]
    PolicyRec one;                  // policy 0 itself: what the kernel reads when the set holds no other (first_row = 0)
    const int* thr;                 // [sum of rungs][6]: the ladders one after another
    unsigned* checked;              // [nslots][stride][4]
    unsigned* state;                // [nslots][kStateWords]
    unsigned* recs;                 // scratch [sum of per][16]
    ethcnn_pacer_result* h_result;  // [nslots], page-locked
};
static_assert(sizeof(FrameTable) < 4096, "the frame table is a kernel argument");

struct BakeSeg {
    unsigned* baked;                // [per][21]
    long rec0;
    int per;
    int first_block;                // of k_pacer_bake_table
    int slot;
    int pad;
};

struct BakeTable {
    BakeSeg seg[kPacerSetMax];
    int nseg;
    const unsigned* recs;
    const unsigned* state;          // [nslots][kStateWords]: a slot's thresholds are its words kStateThr .. kStateThr + 5
};
static_assert(sizeof(BakeTable) < 4096, "the bake table is a kernel argument");

// many: the set holds more than one policy (the kernel form that reads the policy table); else policy 0 from the argument
void launch_table(hipStream_t s, const FrameTable& t, unsigned blocks, bool many);
void launch_bake_table(hipStream_t s, const BakeTable& t, unsigned blocks);

}  // namespace pacer
}  // namespace ethcnn
