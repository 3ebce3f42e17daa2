// ethcnn_sim.h -- shared between the partition-search simulator's kernels (ethcnn_sim.hip) and its host side (ethcnn_sim.cpp):
// include/ethcnn.h "partition-search simulation".
//
// The set in HBM: one 64-byte record per CTU, 16 dwords.  Nodes are numbered 0 (64 x 64), 1 + j (32 x 32 block j) and
// 5 + 4 j + i (16 x 16 block i of block j: QUAD order, not the raster order of the 21 probabilities), so that the children of a node
// are neighbouring bits of a mask.
//   [0, 11)  the 21 bins, 16 bits each, in node order (the 22nd half-word is 0)
//   [11]     inside mask: node lies wholly inside the picture (a decided node when it is visited)
//   [12]     edge mask:   node crosses the frame edge (a node with neither bit lies outside and is never visited)
//   [13]     corner mask: 16 x 16 edge nodes with ONE 8 x 8 inside the picture (the other edge nodes have two)
//   [14]     truth mask:  the node's split flag; bit 31: the CTU is labelled
//   [15]     sub-batch index; 0 = none (per-CTU layout), whose M1 / M2 are kNoGate
// A rejected CTU has empty inside / edge masks: it counts nowhere.  Behind the records, M1 / M2 of every sub-batch as two dwords.
// An add packs into the space behind the set and the host advances the counts only when every piece succeeded and no bad depth byte
// was flagged: a failed add leaves the set as it was.
#pragma once
#include <cstdint>
#include <vector>

#include <hip/hip_runtime_api.h>

namespace ethcnn {
namespace sim {

constexpr int kRecDwords = 16;
constexpr unsigned kL0 = 0x1u, kL1 = 0x1eu, kL2 = 0x1fffe0u;  // the nodes of a level
constexpr unsigned kNoGate = 0x7fffffffu;
constexpr int kFields = 23;             // uint64 words of an ethcnn_sim_counts
constexpr long kMaxSlice = 1L << 24;    // CTUs a lane counts in 32 bits: checked[3] gains up to 64 per CTU
enum { kCallFlag = 0, kCallWhole, kCallLabelled, kCallRejected, kCallWords };

// Frame layout of one launch; per-CTU layout: ctus_w == 0
struct Geom {
    int ctus_w, ctus_h;  // ceil(width / 64), ceil(height / 64)
    int width, height;
    int w16, h16;        // label blocks per row / rows per frame (used with labels only)
    int subs;            // sub-batches per frame
};

// n CTUs from `probs` (frame layout: n = frames * ctus_w * ctus_h; labels NULL or at the first scored label frame) -> recs[0 .. n),
// sub-batches numbered from sub_base, counters into call[kCallWords]
void launch_pack(hipStream_t s, const float* probs, const uint8_t* labels, long n, const Geom& g, unsigned sub_base, unsigned* recs, unsigned* m,
                 unsigned long long* call, int cus);
// out[ncand][kFields] += the counters of cand[ncand][6] (up_k[3], down_k[3]) over recs[0 .. n); out must be zeroed
void launch_eval(hipStream_t s, const unsigned* recs, const unsigned* m, long n, const int* cand, long ncand, int gate_order, unsigned long long* out,
                 int cus);

// a run of whole frames of one geometry inside the set (adjacent adds of the same geometry are one run): what the frame form of
// the partition decisions (ethcnn_decide.h) checks its window against
struct FrameRun {
    int64_t first;  // its first CTU
    int width, height;
    int64_t nframes;
};

}  // namespace sim
}  // namespace ethcnn

struct ethcnn_ctx;
// (the argument rules of the host side: ethcnn_analysis.h)
struct ethcnn_sim {
    ethcnn_ctx* c = nullptr;
    unsigned* d_recs = nullptr;  // [cap_ctus][16]
    unsigned* d_m = nullptr;     // [cap_subs][2]
    int64_t ctus = 0, cap_ctus = 0, subs = 1, cap_subs = 0;  // (sub-batch 0 = none)
    uint64_t whole = 0, labelled = 0, rejected = 0;
    unsigned long long* d_call = nullptr;  // [kCallWords]
    unsigned long long* h_call = nullptr;  // page-locked
    int* d_cand = nullptr;                 // evaluation buffers, grown on demand
    unsigned long long* d_out = nullptr;
    int64_t cap_cand = 0;
    std::vector<ethcnn::sim::FrameRun> runs;  // the frame-layout adds, in set order
    int64_t decide_piece = 0;                 // CTUs per staged piece of ethcnn_decide and ethcnn_budget_bake; 0 = the default
    int* d_budget_thr[2] = {nullptr, nullptr};  // search budget: the ladder and the per-frame thresholds, grown on demand
    int64_t cap_budget_thr[2] = {0, 0};         // (in rows of six ints)
    unsigned* d_rel = nullptr;                  // expected wrong decisions: the reliability table [3][1025] (ethcnn_risk.h); made on first use
};
