// ethcnn_calib.h -- shared between the calibration kernel (ethcnn_calib.hip) and its host side (ethcnn_calib.cpp): include/ethcnn.h
// "threshold calibration".
//
// State of a calibrator in HBM, all uint64 words: the accumulator `acc` and the per-call buffer `call`, each kWords long
//   [0, kHistWords)   hist[level][truth][bin]
//   [kRejected, +3)   rejected[level]
//   [kSkipped]        skipped_partial
// and, behind `call`, the flag word (kFlag): != 0 when a depth byte above 3 was seen.
// A call: zero the flag -> k_calib_count (one launch per piece of the input; LDS histogram per block, flushed into `call` with integer
// atomics) -> k_calib_commit (acc += call unless the flag is up; `call` zeroed either way) -> the flag word to the host.  So a call
// that fails adds nothing, and integer sums make the result independent of grid, order and split.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace ethcnn {
namespace calib {

constexpr int kBins = 1025, kLevels = 3;
constexpr int kHistWords = kLevels * 2 * kBins;  // 6150
constexpr int kRejected = kHistWords, kSkipped = kHistWords + 3, kWords = kHistWords + 4, kFlag = kWords;
constexpr int kTile = 64;                        // CTUs a block stages per trip
constexpr long kMaxCtusPerLaunch = 1L << 26;     // a block's LDS counters are 32-bit: 16 counts a CTU at most

// Frame layout of one launch; per-CTU layout: ctus_w == 0
struct Geom {
    int ctus_w, ctus_h;    // ceil(width / 64), ceil(height / 64)
    int whole_w, whole_h;  // width / 64, height / 64: CTU (cx, cy) is whole when cx < whole_w and cy < whole_h
    int w16, h16;          // label blocks per row / rows per frame
};

// n CTUs (frame layout: n = frames * ctus_w * ctus_h; labels point at the first scored label frame)
void launch_count(hipStream_t s, const float* probs, const uint8_t* labels, long n, const Geom& g, unsigned long long* call, int cus);
void launch_commit(hipStream_t s, unsigned long long* acc, unsigned long long* call);
// ethcnn_calib.cpp: the Thr_info.txt line of six grid values (temp file + rename), behind both writer entries of include/ethcnn.h
int write_thr_line(const char* path, const int32_t down_k[3], const int32_t up_k[3], int order, const char* entry);

}  // namespace calib
}  // namespace ethcnn

struct ethcnn_ctx;
struct ethcnn_calib {
    ethcnn_ctx* c = nullptr;
    unsigned long long* d_state = nullptr;  // acc [kWords] | call [kWords] | flag
    unsigned long long* h_flag = nullptr;   // page-locked
};
