// ethcnn_decide.h -- shared between the kernel of the partition decisions (ethcnn_decide.hip) and its host side (ethcnn_decide.cpp):
// include/ethcnn.h "partition decisions".
//
// Input: the simulator's records (ethcnn_sim.h: 64 bytes a CTU, nodes in QUAD order) and its M1 / M2 table, read as launch_eval reads
// them.  One candidate by value.  Output per CTU, every node and block in the RASTER order of the 21 probabilities:
//   codes [n][24]  bytes 0..20 one code per node, 21 flags, 22 the 8 x 8 CUs that are checked, 23 zero
//   reach [n][16]  bit d of block b: the pruned search can still give block b depth d
//   depth [n][16]  the preferred partition, 0..3, 255 where there is none
//   planes [frames][h16][w16] (frame layout, optional): depth scattered into label planes
// Launch: one lane per CTU, one block of 256 lanes per 256 CTUs, no grid-stride loop (a block stages its 6144 code bytes in LDS and
// needs one barrier).  A lane loads its record as four uint4; reach and depth leave as one uint4 per lane when the buffer is 16-byte
// aligned (four dwords else); the codes go through LDS so that a wave stores 64 consecutive dwords; a plane row is one dword where
// the row's four blocks lie in the picture and the address is aligned, bytes else.  No atomics: every output byte has one writer.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace ethcnn {
namespace decide {

constexpr int kCodeBytes = 24, kBlockBytes = 16;
constexpr int kOutBytes = kCodeBytes + 2 * kBlockBytes;  // per CTU, all three outputs

struct Cand {
    int up[3], down[3];
    int gate_order;  // ETHCNN_SIM_GATES_*
    int mid;         // a BOTH node of the preferred partition splits <=> bin > mid
};

// label planes of the launch's frames; p == nullptr: none.  The launch's n must then be frames * ctus_w * ctus_h.
struct Planes {
    uint8_t* p;
    int ctus_w, ctus_h;
    int w16, h16;
};

// recs: the record of the launch's first CTU.  codes / reach / depth may be nullptr (4-byte aligned else); every output is indexed
// from the launch's first CTU.
void launch_decide(hipStream_t s, const unsigned* recs, const unsigned* m, long n, const Cand& c, const Planes& pl, uint8_t* codes, uint8_t* reach,
                   uint8_t* depth);

}  // namespace decide
}  // namespace ethcnn
