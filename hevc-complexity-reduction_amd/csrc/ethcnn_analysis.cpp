// ethcnn_analysis.cpp -- the shared host routines of the threshold-analysis family (ethcnn_analysis.h).
#include "ethcnn_analysis.h"
#include "ethcnn_budget.h"

namespace ethcnn {
namespace sim {
int check_cand(ethcnn_ctx* c, const ethcnn_sim_thr& t, long long at) {
    for (int l = 0; l < 3; ++l)
        if (t.up_k[l] < 0 || t.up_k[l] > 1024 || t.down_k[l] < -1 || t.down_k[l] > 1024)
            return set_err(c, ETHCNN_ERR_ARG, "candidate %lld, level %d: up_k = %d / down_k = %d outside 0..1024 / -1..1024", at, l + 1, t.up_k[l], t.down_k[l]);
    return 0;
}

int check_gates(ethcnn_ctx* c, int gate_order) {
    if (gate_order != ETHCNN_SIM_GATES_NONE && gate_order != ETHCNN_SIM_GATES_AI && gate_order != ETHCNN_SIM_GATES_LDP)
        return set_err(c, ETHCNN_ERR_ARG, "gate order %d is none of ETHCNN_SIM_GATES_NONE / _AI / _LDP", gate_order);
    return 0;
}

int check_frame_run(ethcnn_sim* k, int64_t first, int width, int height, int64_t nframes) {
    const int64_t per = (int64_t)((width + 63) / 64) * ((height + 63) / 64);
    for (const FrameRun& r : k->runs)
        if (r.width == width && r.height == height && first >= r.first && (first - r.first) % per == 0 && (first - r.first) / per <= r.nframes &&
            nframes <= r.nframes - (first - r.first) / per)
            return 0;
    return set_err(k->c, ETHCNN_ERR_ARG, "CTU %lld + %lld frames do not lie on the frame boundaries of CTUs added as %d x %d frames", (long long)first,
                   (long long)nframes, width, height);
}

int check_size(ethcnn_ctx* c, int width, int height, int unit, PicSize* s) {
    if (width <= 0 || height <= 0 || width > 65536 || height > 65536 || width % unit || height % unit)
        return set_err(c, ETHCNN_ERR_ARG, "%s (up to 65536): got %d x %d",
                       unit == 16 ? "label files exist for sizes that are multiples of 16" : "HM pictures have sizes that are multiples of 8", width, height);
    *s = PicSize{(width + 63) / 64, (height + 63) / 64, width / 16, height / 16};
    return 0;
}

int check_weights(ethcnn_ctx* c, const uint64_t* weight, const char* entry) {
    if (weight)
        for (int d = 0; d < 4; ++d)
            if (weight[d] >> 32) return set_err(c, ETHCNN_ERR_ARG, "%sweight[%d] = %llu is not below 2^32", entry, d, (unsigned long long)weight[d]);
    return 0;
}

int check_rung_count(ethcnn_ctx* c, int64_t n, const char* entry, const char* name) {
    if (n < 1 || n > budget::kMaxRungs) return set_err(c, ETHCNN_ERR_ARG, "%sa ladder has 1..%d rungs: got %s%lld", entry, budget::kMaxRungs, name, (long long)n);
    return 0;
}

bool cost_fits(int64_t ctus, const uint64_t w[4]) {
    return !(((u128)ctus * ((u128)w[0] + (u128)4 * w[1] + (u128)16 * w[2] + (u128)64 * w[3])) >> 64);
}
}  // namespace sim

int Scratch::alloc(ethcnn_ctx* c, size_t bytes, const char* what, bool check_free) {
    size_t free_b = 0, total_b = 0;
    if (check_free) HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    if ((check_free && bytes > free_b) || hipMalloc((void**)&p_, bytes) != hipSuccess) {
        (void)hipGetLastError();
        p_ = nullptr;
        return set_err(c, ETHCNN_ERR_NOMEM, "%s: %llu bytes of scratch do not fit in device memory", what, (unsigned long long)bytes);
    }
    return 0;
}

int stage_pieces(ethcnn_ctx* c, Scratch& stage, const char* what, const float* probs, const uint8_t* labels, int64_t units, int64_t piece, int64_t pb,
                 int64_t lb, const StageFn& fn) {
    piece = std::min(piece, units);
    const size_t label_at = ((size_t)(piece * pb) + 255) / 256 * 256;  // probabilities, then labels: one allocation
    if (int rc = stage.alloc(c, label_at + (labels ? (size_t)(piece * lb) : 0), what)) return rc;
    uint8_t* const d_l = labels ? stage.at(label_at) : nullptr;
    for (int64_t at = 0; at < units; at += piece) {
        const int64_t m = std::min(piece, units - at);
        hipError_t e = hipMemcpyAsync(stage.at(), (const uint8_t*)probs + at * pb, (size_t)(m * pb), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && labels) e = hipMemcpyAsync(d_l, labels + at * lb, (size_t)(m * lb), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return set_err(c, ETHCNN_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
        if (int rc = fn(stage.at<float>(), d_l, m)) return rc;
    }
    return 0;
}

int write_text_atomic(const char* path, const std::string& text) {
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long)getpid());
    FILE* f = std::fopen(tmp.c_str(), "w");
    if (!f) return set_err(nullptr, ETHCNN_ERR_IO, "cannot open %s for writing: %s", tmp.c_str(), std::strerror(errno));
    int rc = 0;
    if (std::fwrite(text.data(), 1, text.size(), f) != text.size()) rc = set_err(nullptr, ETHCNN_ERR_IO, "write to %s failed: %s", tmp.c_str(), std::strerror(errno));
    if (std::fclose(f) != 0 && !rc) rc = set_err(nullptr, ETHCNN_ERR_IO, "close of %s failed", tmp.c_str());
    if (!rc && std::rename(tmp.c_str(), path) != 0) rc = set_err(nullptr, ETHCNN_ERR_IO, "rename %s -> %s failed: %s", tmp.c_str(), path, std::strerror(errno));
    if (rc) std::remove(tmp.c_str());
    return rc;
}

std::string thr_line(const int32_t down_k[3], const int32_t up_k[3], int order) {
    double v[6];
    for (int l = 0; l < 3; ++l) {
        v[2 * l + (order == ETHCNN_THR_ORDER_AI ? 1 : 0)] = down_k[l] / 1024.0;
        v[2 * l + (order == ETHCNN_THR_ORDER_AI ? 0 : 1)] = up_k[l] / 1024.0;
    }
    char line[128];
    std::snprintf(line, sizeof line, "%.10f %.10f %.10f %.10f %.10f %.10f\n", v[0], v[1], v[2], v[3], v[4], v[5]);
    return line;
}

}  // namespace ethcnn
