// ethcnn_budget.h -- shared between the kernels of the search budget (ethcnn_budget.hip) and their host side (ethcnn_budget.cpp):
// include/ethcnn.h "search budget".
//
// Input of both kernels: the simulator's records (ethcnn_sim.h: 64 bytes a CTU, nodes in QUAD order) of a window of whole frames of
// one geometry, `per` CTUs a frame.  The gates are always open (ETHCNN_SIM_GATES_NONE), so the M1 / M2 table is not read.
//
// k_budget_cost: thr int [rungs][6] (up_k[3], down_k[3]; the host appends the full search as the last rung) ->
//   checked uint32 [nframes][rungs][4], which the host zeroes first.
//   Launch: a lane is a rung, a wave owns 64 rungs and a slice of ONE frame's CTUs (blocks of 256 lanes = 4 waves; wave index ->
//   rung group fastest, then slice, then frame).  The record address is the same for the whole wave, so the record arrives by uniform
//   loads, as in k_sim_eval; a lane keeps its six thresholds and four 32-bit counters in registers and adds them to its words with
//   integer atomics at the end of its slice (one add per word when a frame is one slice).  Lanes past the last rung write nothing.
//
// k_budget_bake: thr int [nframes][6] (the thresholds of each frame's rung) -> probs float [n][21], RASTER order.
//   Launch: a lane is a CTU, a block 256 consecutive CTUs (usually of several frames: a lane takes its thresholds from the row of
//   ITS frame), no grid-stride loop.  A block stages its 256 x 21 dwords in LDS (21504 bytes; the row stride of 21 dwords is odd, so
//   the lanes of a wave hit different banks) and stores them as consecutive dwords after one barrier.  The three values are bit
//   patterns: no float arithmetic.  Every output dword has one writer.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace ethcnn {
namespace budget {

constexpr int kNout = 21;
constexpr int kMaxRungs = 4096;
constexpr int kDefaultRungs = 513;
constexpr long kMaxFrameCtus = 1L << 24;  // CTUs of a frame that a lane counts in 32 bits: checked[3] gains up to 64 per CTU

// recs: the record of the window's first CTU; d_checked [nframes][rungs][4] zeroed by the caller
void launch_cost(hipStream_t s, const unsigned* recs, long per, long nframes, const int* d_thr, int rungs, unsigned* d_checked, int cus);
// CTUs ctu0 .. ctu0 + n of the window (frame of a CTU = its index in the window / per); d_probs is indexed from ctu0
void launch_bake(hipStream_t s, const unsigned* recs, long per, long ctu0, long n, const int* d_frame_thr, float* d_probs);

}  // namespace budget
}  // namespace ethcnn
