// ethcnn_analysis.h -- host only: what the host files of the threshold-analysis family (calibrator, simulator, decisions, budget,
// pacer, ladder, audit, expected wrong decisions) share: constants, argument rules, the per-call device scratch, the staging of host
// arrays in pieces and the text-file writer.  Definitions: ethcnn_analysis.cpp.
#pragma once
#include "ethcnn_ctx.h"
#include "ethcnn_sim.h"

typedef unsigned __int128 u128;

inline int cus_of(const ethcnn_ctx* c) { return c->cus > 0 ? c->cus : 256; }

namespace ethcnn {
namespace sim {

constexpr int64_t kStageCtus = 1 << 20;             // CTUs per staged piece of the host entries (100 MB of device memory)
constexpr uint64_t kDefaultWeight[4] = {64, 16, 4, 1};
constexpr ethcnn_sim_thr kFullSearch = {{1024, 1024, 1024}, {-1, -1, -1}};  // every CU of every size is checked

// ---- argument rules: 0, or ETHCNN_ERR_ARG with the message set; c may be NULL (the message then goes where ethcnn_last_error(NULL) reads)
int check_cand(ethcnn_ctx* c, const ethcnn_sim_thr& t, long long at);
int check_gates(ethcnn_ctx* c, int gate_order);
// the window rule of the frame forms (ethcnn_decide_frames_device, ethcnn_budget_*): nframes whole frames from CTU `first` on lie
// inside one run of width x height frames, `first` on a frame boundary of it
int check_frame_run(ethcnn_sim* k, int64_t first, int width, int height, int64_t nframes);

struct PicSize {
    int ctus_w, ctus_h;  // ceil(width / 64), ceil(height / 64)
    int w16, h16;        // label blocks per row / rows per frame
    int64_t ctus() const { return (int64_t)ctus_w * ctus_h; }
};
// width and height are multiples of `unit` up to 65536: 8 for HM pictures, 16 where label files go with them
int check_size(ethcnn_ctx* c, int width, int height, int unit, PicSize* s);
// weight (may be NULL: the defaults) holds values below 2^32; the message starts with `entry`
int check_weights(ethcnn_ctx* c, const uint64_t* weight, const char* entry = "");
// a ladder of n rungs; the message starts with `entry` and calls the count `name`
int check_rung_count(ethcnn_ctx* c, int64_t n, const char* entry = "", const char* name = "");
// a CTU has at most 1, 4, 16 and 64 checked CUs of the four sizes: whether the largest cost `ctus` CTUs can have fits in 64 bits
bool cost_fits(int64_t ctus, const uint64_t weight[4]);

}  // namespace sim

// Device scratch of one call: freed when the call returns, whichever way.
class Scratch {
public:
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        if (p_) (void)hipFree(p_);
    }
    // 0, or ETHCNN_ERR_NOMEM "<what>: <bytes> bytes ..." with HIP's sticky error cleared.  check_free: what hipMemGetInfo reports as not
    // fitting is refused without asking for it
    int alloc(ethcnn_ctx* c, size_t bytes, const char* what, bool check_free = false);
    template <class T = uint8_t>
    T* at(size_t byte_offset = 0) const {
        return reinterpret_cast<T*>(p_ + byte_offset);
    }
    // the allocation becomes the caller's
    template <class T>
    T* release() {
        T* p = at<T>();
        p_ = nullptr;
        return p;
    }

private:
    uint8_t* p_ = nullptr;
};

// Host arrays to the device in pieces: `units` (CTUs, or frames) of pb bytes of probabilities and, where labels is not NULL, lb bytes of
// labels each go through `stage`, `piece` units at a time; fn(d_probs, d_labels, m) is called with the copies of m units queued on the
// context's stream (the copies of the next piece wait, in stream order, for what fn launched).  The first non-zero return ends the loop.
typedef std::function<int(const float* d_probs, const uint8_t* d_labels, int64_t m)> StageFn;
int stage_pieces(ethcnn_ctx* c, Scratch& stage, const char* what, const float* probs, const uint8_t* labels, int64_t units, int64_t piece, int64_t pb,
                 int64_t lb, const StageFn& fn);

// text -> path through a temporary file beside it and a rename: never a partial file.  0, or ETHCNN_ERR_IO (message at
// ethcnn_last_error(NULL)) with no temporary file left
int write_text_atomic(const char* path, const std::string& text);
// a Thr_info line: six grid values in the order the All-Intra encoder (up, down per level) or the Low-Delay-P one (down, up) reads them
//   HM-16.5_Test_AI/source/Lib/TLibEncoder/TEncCu.cpp:250       fscanf("%f %f %f %f %f %f", &fUp[0], &fDown[0], &fUp[1], &fDown[1], &fUp[2], &fDown[2])
//   HM-16.5_Test_LDP/source/Lib/TLibEncoder/TEncGOP.cpp:1449    fscanf("%f %f %f %f %f %f", &fDown[0], &fUp[0], &fDown[1], &fUp[1], &fDown[2], &fUp[2])
std::string thr_line(const int32_t down_k[3], const int32_t up_k[3], int order);

}  // namespace ethcnn
