// ethcnn_pacer_set_plan.h -- internal: the layout of one ethcnn_pacer_set_frames call (include/ethcnn.h, ethcnn_pacer_set_plan).
// Host only, no HIP: ethcnn_pacer_set_plan.cpp is also compiled into a stand-alone program (tools/pacer_set_plan_check.cpp).
#pragma once
#include <cstdint>

constexpr int kPacerSetMax = 32;                   // slots of a set = frames of a call
constexpr int kPacerSetSliceCtus = 64;             // pacer::kSliceCtus: CTUs of a slice at most
constexpr int kPacerSetThreads = 256;              // lanes of a block of both kernels: rungs of a rung block, CTUs of a bake block
constexpr int64_t kPacerSetMaxFrameCtus = 1 << 24; // budget::kMaxFrameCtus: a frame has fewer
constexpr int64_t kPacerSetMaxRungs = 4096;        // budget::kMaxRungs

struct PacerSetSeg {
    int64_t count_first, count_blocks;  // blocks of k_pacer_table: slices x rung blocks, rung block fastest
    int64_t bake_first, bake_blocks;    // blocks of k_pacer_bake_table: 256 CTUs each
    int64_t rec0;                       // its first record in the shared scratch
    int slice_len;                      // CTUs of its slices (the last one may be shorter)
};

// n frames of nctus[j] CTUs under K + 1 rungs, in call order -> seg[n] and both grid sizes.  0, or ETHCNN_ERR_ARG (n outside 1..32, a
// frame of no or of 2^24 or more CTUs, K outside 1..4096) with nothing written.
int pacer_set_layout(const int64_t* nctus, int n, int64_t K, PacerSetSeg* seg, int64_t* count_grid, int64_t* bake_grid);
// the same with rungs of its own per frame: frame j under K[j] + 1 rungs (the ladder of its slot's policy), so that a frame's count blocks
// are slices x ceil((K[j] + 1) / 256).  Refuses per frame what pacer_set_layout refuses, and a NULL K.
int pacer_set_layout_rungs(const int64_t* nctus, const int64_t* K, int n, PacerSetSeg* seg, int64_t* count_grid, int64_t* bake_grid);
