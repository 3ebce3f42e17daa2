// ethcnn_audit.h -- shared between the comparison kernel (ethcnn_audit.hip) and its host side (ethcnn_audit.cpp): include/ethcnn.h
// "comparing two predictions".
//
// The call state in HBM: kWords uint64 words that one or more launches add to.  Sums are added with one 64-bit atomic per block and
// non-zero counter; the three maxima are 64-bit words (bits of |a - b|) << 32 | ~index, reduced with atomicMax: |a - b| >= 0, so its bits
// order as integers, and of two equal values the LOWER index has the larger complement.  0 = nothing compared on that level (an index is
// below 2^31, so the complement of a compared value is never 0).
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace ethcnn {
namespace audit {

constexpr int kTile = 256;  // CTUs a block stages per trip: one lane per CTU, 2 x 21504 bytes of LDS
enum {
    kRejected = 0,
    kOverTol = 1,     // [3]
    kBitsDiff = 4,    // [3]
    kClassDiff = 7,   // [3]
    kSearchDiff = 10,
    kCheckedA = 11,   // [4]
    kCheckedB = 15,   // [4]
    kSums = 19,
    kMax = 19,        // [3] packed maxima
    kWords = 22
};

// Frame layout of one launch; per-CTU layout: ctus_w == 0 (every node is a decided node)
struct Geom {
    int ctus_w, ctus_h;  // ceil(width / 64), ceil(height / 64)
    int width, height;
};

// thr: up_k[3], down_k[3]; has_thr == 0: the fields that need a candidate are not computed
struct Thr {
    int up[3], down[3];
    int has_thr;
};

// the grid of one launch over n CTUs on a device of `cus` compute units: min(tiles, 3 * cus).  Three blocks a CU is what both the LDS
// (43 KB a block) and the registers (168 a lane) allow, so every block of a capped grid is resident at once and the blocks walk the tiles
// side by side; a fourth block a CU would start when the first ones end and run its trips on a third of the machine.
inline int grid_for(long n, int cus) {
    const long tiles = (n + kTile - 1) / kTile;
    return (int)(tiles < 3L * cus ? tiles : 3L * cus);
}

// words[kWords] += the comparison of a[0 .. n) with b[0 .. n), whose first CTU has index `first` (of the call, and of the frame run in
// the frame layout); flags (may be NULL) [n] bytes.  a, b: any 4-byte aligned address.
void launch_compare(hipStream_t s, const float* a, const float* b, long n, long first, const Geom& g, float tol, const Thr& thr,
                    unsigned long long* words, uint8_t* flags, int cus);

}  // namespace audit
}  // namespace ethcnn
