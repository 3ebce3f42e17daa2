// ethcnn_pacer_set_plan.cpp -- the host-only entry of ethcnn_pacer_set_* (include/ethcnn.h): the layout of a call, shared by the launch
// code (ethcnn_pacer_set.cpp) and the tests.  No HIP in this file (ethcnn_pacer_set_plan.h).  Everything is summed in 64 bits: 32 frames
// of 2^24 - 1 CTUs are 2^29 records of 64 bytes.
#include "ethcnn_pacer_set_plan.h"

#include "../../include/ethcnn.h"

int pacer_set_layout_rungs(const int64_t* nctus, const int64_t* K, int n, PacerSetSeg* seg, int64_t* count_grid, int64_t* bake_grid) {
    if (!nctus || !K || !seg || n < 1 || n > kPacerSetMax) return ETHCNN_ERR_ARG;
    for (int j = 0; j < n; ++j)
        if (nctus[j] < 1 || nctus[j] >= kPacerSetMaxFrameCtus || K[j] < 1 || K[j] > kPacerSetMaxRungs) return ETHCNN_ERR_ARG;
    int64_t count = 0, bake = 0, rec = 0;
    for (int j = 0; j < n; ++j) {
        // slices of at most kPacerSetSliceCtus CTUs, balanced, as pacer::launch_frame cuts them; each under every rung block of ITS ladder
        const int64_t per = nctus[j], most = (per + kPacerSetSliceCtus - 1) / kPacerSetSliceCtus;
        const int64_t slice_len = (per + most - 1) / most, slices = (per + slice_len - 1) / slice_len;
        const int64_t rung_blocks = (K[j] + 1 + kPacerSetThreads - 1) / kPacerSetThreads;
        PacerSetSeg& s = seg[j];
        s.count_first = count, s.count_blocks = slices * rung_blocks;
        s.bake_first = bake, s.bake_blocks = (per + kPacerSetThreads - 1) / kPacerSetThreads;
        s.rec0 = rec;
        s.slice_len = (int)slice_len;
        count += s.count_blocks, bake += s.bake_blocks, rec += per;
    }
    if (count_grid) *count_grid = count;  // (at most 32 x 2^18 x 17 < 2^31: a grid's x extent)
    if (bake_grid) *bake_grid = bake;
    return 0;
}

int pacer_set_layout(const int64_t* nctus, int n, int64_t K, PacerSetSeg* seg, int64_t* count_grid, int64_t* bake_grid) {
    int64_t each[kPacerSetMax];
    for (int j = 0; j < kPacerSetMax; ++j) each[j] = K;
    return pacer_set_layout_rungs(nctus, each, n, seg, count_grid, bake_grid);
}

namespace {
int plan_out(const PacerSetSeg* seg, int n, int64_t count, int64_t bake, int64_t* count_first_out, int64_t* count_blocks_out, int32_t* slice_len_out,
             int64_t* bake_first_out, int64_t* rec0_out, int64_t* count_grid_out, int64_t* bake_grid_out) {
    for (int j = 0; j < n; ++j) {
        if (count_first_out) count_first_out[j] = seg[j].count_first;
        if (count_blocks_out) count_blocks_out[j] = seg[j].count_blocks;
        if (slice_len_out) slice_len_out[j] = seg[j].slice_len;
        if (bake_first_out) bake_first_out[j] = seg[j].bake_first;
        if (rec0_out) rec0_out[j] = seg[j].rec0;
    }
    if (count_grid_out) *count_grid_out = count;
    if (bake_grid_out) *bake_grid_out = bake;
    return ETHCNN_OK;
}
}  // namespace

extern "C" int ethcnn_pacer_set_plan(const int64_t* nctus, int n, int64_t K, int64_t* count_first_out, int64_t* count_blocks_out, int32_t* slice_len_out,
                                     int64_t* bake_first_out, int64_t* rec0_out, int64_t* count_grid_out, int64_t* bake_grid_out) {
    PacerSetSeg seg[kPacerSetMax];
    int64_t count = 0, bake = 0;
    if (pacer_set_layout(nctus, n, K, seg, &count, &bake)) return ETHCNN_ERR_ARG;
    return plan_out(seg, n, count, bake, count_first_out, count_blocks_out, slice_len_out, bake_first_out, rec0_out, count_grid_out, bake_grid_out);
}

extern "C" int ethcnn_pacer_policies_plan(const int64_t* nctus, const int64_t* K, int n, int64_t* count_first_out, int64_t* count_blocks_out,
                                           int32_t* slice_len_out, int64_t* bake_first_out, int64_t* rec0_out, int64_t* count_grid_out,
                                           int64_t* bake_grid_out) {
    PacerSetSeg seg[kPacerSetMax];
    int64_t count = 0, bake = 0;
    if (pacer_set_layout_rungs(nctus, K, n, seg, &count, &bake)) return ETHCNN_ERR_ARG;
    return plan_out(seg, n, count, bake, count_first_out, count_blocks_out, slice_len_out, bake_first_out, rec0_out, count_grid_out, bake_grid_out);
}
