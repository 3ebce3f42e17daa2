// ethcnn_calib.cpp -- host side of the threshold calibrator (include/ethcnn.h "threshold calibration"): the calibrator object and its
// add / get entries around the kernel of ethcnn_calib.hip, and the two context-free entries: the choice of the six thresholds from a
// histogram and the Thr_info.txt writer.
#include "ethcnn_analysis.h"
#include "ethcnn_calib.h"

using namespace ethcnn::calib;
using ethcnn::sim::kStageCtus;

namespace {
constexpr size_t kStateBytes = (size_t)(2 * kWords + 1) * 8;

unsigned long long* acc_of(ethcnn_calib* k) { return k->d_state; }
unsigned long long* call_of(ethcnn_calib* k) { return k->d_state + kWords; }

int begin(ethcnn_calib* k) {
    ethcnn_ctx* c = k->c;
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;  // the context's completion word does not cover these launches
    HIPCHK(c, hipMemsetAsync(call_of(k) + kFlag, 0, 8, c->stream));
    return 0;
}

// after a failed HIP call in the middle of an add: whatever the launches so far counted must not reach the accumulator
void discard(ethcnn_calib* k) {
    (void)hipGetLastError();
    (void)hipMemsetAsync(call_of(k), 0, (size_t)(kWords + 1) * 8, k->c->stream);
    (void)hipStreamSynchronize(k->c->stream);
}

int finish(ethcnn_calib* k) {
    ethcnn_ctx* c = k->c;
    launch_commit(c->stream, acc_of(k), call_of(k));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(k->h_flag, call_of(k) + kFlag, 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        discard(k);
        return set_err(c, ETHCNN_ERR_DEVICE, "calibration: %s", hipGetErrorString(e));
    }
    if (*k->h_flag)
        return set_err(c, ETHCNN_ERR_FORMAT, "%llu CTU(s) hold a depth byte above 3 (CU depths are 0..3); nothing was added", *k->h_flag);
    return ETHCNN_OK;
}

// launches over n CTUs (per-CTU layout) or nframes frames (frame layout) that are in HBM
hipError_t count_device(ethcnn_calib* k, const float* d_probs, const uint8_t* d_labels, int64_t n, const Geom& g) {
    ethcnn_ctx* c = k->c;
    if (g.ctus_w == 0) {
        for (int64_t at = 0; at < n; at += kMaxCtusPerLaunch)
            launch_count(c->stream, d_probs + at * 21, d_labels + at * 16, (long)std::min<int64_t>(kMaxCtusPerLaunch, n - at), g, call_of(k), cus_of(c));
    } else {
        const int64_t per = (int64_t)g.ctus_w * g.ctus_h, lab = (int64_t)g.w16 * g.h16, step = std::max<int64_t>(1, kMaxCtusPerLaunch / per);
        for (int64_t f = 0; f < n; f += step)
            launch_count(c->stream, d_probs + f * per * 21, d_labels + f * lab, (long)(std::min(step, n - f) * per), g, call_of(k), cus_of(c));
    }
    return hipGetLastError();
}

int calib_geom(ethcnn_ctx* c, int width, int height, Geom* g) {
    ethcnn::sim::PicSize s;
    if (int rc = ethcnn::sim::check_size(c, width, height, 16, &s)) return rc;
    *g = Geom{s.ctus_w, s.ctus_h, width / 64, height / 64, s.w16, s.h16};
    return 0;
}

// host pointers: pieces of `units` (CTUs, or frames) go through a device buffer; pb / lb = bytes of probabilities / labels per unit
int add_staged(ethcnn_calib* k, const float* probs, const uint8_t* labels, int64_t units, int64_t piece, int64_t pb, int64_t lb, const Geom& g) {
    ethcnn_ctx* c = k->c;
    if (int rc = begin(k)) return rc;
    Scratch stage;
    const int rc = stage_pieces(c, stage, "calibration", probs, labels, units, piece, pb, lb, [&](const float* d_p, const uint8_t* d_l, int64_t m) {
        const hipError_t e = count_device(k, d_p, d_l, m, g);
        return e == hipSuccess ? 0 : set_err(c, ETHCNN_ERR_DEVICE, "calibration: %s", hipGetErrorString(e));
    });
    if (rc == ETHCNN_ERR_DEVICE) discard(k);
    return rc ? rc : finish(k);
}
}  // namespace

extern "C" int ethcnn_calib_create(ethcnn_ctx* c, ethcnn_calib** out) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "null output pointer");
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    ethcnn_calib* k = new (std::nothrow) ethcnn_calib;
    if (!k) return set_err(c, ETHCNN_ERR_NOMEM, "out of memory");
    k->c = c;
    hipError_t e = hipMalloc((void**)&k->d_state, kStateBytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&k->h_flag, 8, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemsetAsync(k->d_state, 0, kStateBytes, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ethcnn_calib_destroy(k);
        return set_err(c, ETHCNN_ERR_DEVICE, "calibrator: %s", hipGetErrorString(e));
    }
    *out = k;
    return ETHCNN_OK;
}

extern "C" void ethcnn_calib_destroy(ethcnn_calib* k) {
    if (!k) return;
    (void)hipSetDevice(k->c->device);
    if (k->d_state) {
        (void)hipStreamSynchronize(k->c->stream);
        (void)hipFree(k->d_state);
    }
    if (k->h_flag) (void)hipHostFree(k->h_flag);
    delete k;
}

extern "C" int ethcnn_calib_reset(ethcnn_calib* k) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;
    HIPCHK(c, hipMemsetAsync(k->d_state, 0, kStateBytes, c->stream));
    return ETHCNN_OK;
}

extern "C" int ethcnn_calib_add_device(ethcnn_calib* k, const float* d_probs, const uint8_t* d_depth16, int64_t n) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (n < 0) return set_err(c, ETHCNN_ERR_ARG, "negative CTU count %lld", (long long)n);
    if (n == 0) return ETHCNN_OK;
    if (!d_probs || !d_depth16 || ((uintptr_t)d_probs | (uintptr_t)d_depth16) % 4) return set_err(c, ETHCNN_ERR_ARG, "null or not 4-byte aligned device buffer");
    if (int rc = begin(k)) return rc;
    const Geom g = {0, 0, 0, 0, 0, 0};
    const hipError_t e = count_device(k, d_probs, d_depth16, n, g);
    if (e != hipSuccess) {
        discard(k);
        return set_err(c, ETHCNN_ERR_DEVICE, "calibration: %s", hipGetErrorString(e));
    }
    return finish(k);
}

extern "C" int ethcnn_calib_add(ethcnn_calib* k, const float* probs, const uint8_t* depth16, int64_t n) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (n < 0) return set_err(c, ETHCNN_ERR_ARG, "negative CTU count %lld", (long long)n);
    if (n == 0) return ETHCNN_OK;
    if (!probs || !depth16) return set_err(c, ETHCNN_ERR_ARG, "null buffer");
    const Geom g = {0, 0, 0, 0, 0, 0};
    return add_staged(k, probs, depth16, n, kStageCtus, 84, 16, g);
}

extern "C" int ethcnn_calib_add_frames_device(ethcnn_calib* k, const float* d_probs, const uint8_t* d_labels, int width, int height,
                                              int64_t nframes, int64_t skip_label_frames) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    Geom g;
    if (int rc = calib_geom(c, width, height, &g)) return rc;
    if (nframes < 0 || skip_label_frames < 0) return set_err(c, ETHCNN_ERR_ARG, "negative frame count");
    if (nframes == 0) return ETHCNN_OK;
    if (!d_probs || !d_labels || (uintptr_t)d_probs % 4) return set_err(c, ETHCNN_ERR_ARG, "null or misaligned device buffer");
    if (int rc = begin(k)) return rc;
    const hipError_t e = count_device(k, d_probs, d_labels + skip_label_frames * g.w16 * g.h16, nframes, g);
    if (e != hipSuccess) {
        discard(k);
        return set_err(c, ETHCNN_ERR_DEVICE, "calibration: %s", hipGetErrorString(e));
    }
    return finish(k);
}

extern "C" int ethcnn_calib_add_frames(ethcnn_calib* k, const float* probs, const uint8_t* labels, int width, int height, int64_t nframes,
                                       int64_t skip_label_frames) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    Geom g;
    if (int rc = calib_geom(c, width, height, &g)) return rc;
    if (nframes < 0 || skip_label_frames < 0) return set_err(c, ETHCNN_ERR_ARG, "negative frame count");
    if (nframes == 0) return ETHCNN_OK;
    if (!probs || !labels) return set_err(c, ETHCNN_ERR_ARG, "null buffer");
    const int64_t per = (int64_t)g.ctus_w * g.ctus_h, lab = (int64_t)g.w16 * g.h16;
    return add_staged(k, probs, labels + skip_label_frames * lab, nframes, std::max<int64_t>(1, kStageCtus / per), per * 84, lab, g);
}

extern "C" int ethcnn_calib_get(ethcnn_calib* k, uint64_t* hist, uint64_t rejected[3], uint64_t* skipped_partial) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<unsigned long long> w((size_t)kWords);
    HIPCHK(c, hipMemcpyAsync(w.data(), acc_of(k), (size_t)kWords * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hist) std::copy(w.begin(), w.begin() + kHistWords, hist);
    if (rejected) std::copy(w.begin() + kRejected, w.begin() + kRejected + 3, rejected);
    if (skipped_partial) *skipped_partial = w[kSkipped];
    return ETHCNN_OK;
}

// ---- the choice: integers only (128-bit products), see include/ethcnn.h
extern "C" int ethcnn_calib_choose(const uint64_t* hist, const uint32_t eps_down_ppm[3], const uint32_t eps_up_ppm[3], ethcnn_calib_report* rep) {
    if (!hist || !eps_down_ppm || !eps_up_ppm || !rep) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_calib_choose: null argument");
    for (int l = 0; l < 3; ++l)
        if (eps_down_ppm[l] > 1000000u || eps_up_ppm[l] > 1000000u)
            return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_calib_choose: a budget is in parts per million, 0..1000000 (level %d: %u / %u)", l + 1,
                           eps_down_ppm[l], eps_up_ppm[l]);
    for (int l = 0; l < 3; ++l) {
        const uint64_t *h0 = hist + (size_t)(l * 2) * kBins, *h1 = h0 + kBins;
        // c0[k + 1] / c1[k + 1] = samples with bin <= k, k = -1 .. 1024
        uint64_t c0[kBins + 1], c1[kBins + 1];
        c0[0] = c1[0] = 0;
        for (int b = 0; b < kBins; ++b) {
            c0[b + 1] = c0[b] + h0[b];
            c1[b + 1] = c1[b] + h1[b];
        }
        const uint64_t n0 = c0[kBins], n1 = c1[kBins];
        auto miss = [&](int k) { return c1[k + 1]; };
        auto fsplit = [&](int k) { return n0 - c0[k + 1]; };
        int down = -1, up = kBins - 1;
        while (down < kBins - 1 && (u128)miss(down + 1) * 1000000u <= (u128)eps_down_ppm[l] * n1) ++down;
        while (up > 0 && (u128)fsplit(up - 1) * 1000000u <= (u128)eps_up_ppm[l] * n0) --up;
        ethcnn_calib_level& r = rep->level[l];
        r.crossed = down > up;
        if (r.crossed) {
            int best = up;
            for (int k = up + 1; k <= down; ++k)
                if (miss(k) + fsplit(k) < miss(best) + fsplit(best)) best = k;
            down = up = best;
        }
        r.n0 = n0;
        r.n1 = n1;
        r.down_k = down;
        r.up_k = up;
        r.down = down / 1024.0;
        r.up = up / 1024.0;
        r.miss = miss(down);
        r.fsplit = fsplit(up);
        r.uncertain = c0[up + 1] + c1[up + 1] - c0[down + 1] - c1[down + 1];
        r.uncertain_share = n0 + n1 ? (double)r.uncertain / (double)(n0 + n1) : 0.0;
        r.accuracy_512 = n0 + n1 ? (double)(c0[513] + (n1 - c1[513])) / (double)(n0 + n1) : 0.0;
        r.empty_class = n0 == 0 || n1 == 0;
    }
    return ETHCNN_OK;
}

int ethcnn::calib::write_thr_line(const char* path, const int32_t down_k[3], const int32_t up_k[3], int order, const char* entry) {
    if (order != ETHCNN_THR_ORDER_AI && order != ETHCNN_THR_ORDER_LDP)
        return set_err(nullptr, ETHCNN_ERR_ARG, "%s: order %d is neither ETHCNN_THR_ORDER_AI nor ETHCNN_THR_ORDER_LDP", entry, order);
    for (int l = 0; l < 3; ++l)
        if (down_k[l] < -1 || down_k[l] > 1024 || up_k[l] < 0 || up_k[l] > 1024)
            return set_err(nullptr, ETHCNN_ERR_ARG, "%s: level %d holds k = %d / %d outside -1..1024 / 0..1024", entry, l + 1, down_k[l], up_k[l]);
    return write_text_atomic(path, thr_line(down_k, up_k, order));
}

extern "C" int ethcnn_calib_write_thr_info(const char* path, const ethcnn_calib_report* rep, int order) {
    if (!path || !rep) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_calib_write_thr_info: null argument");
    const int32_t down_k[3] = {rep->level[0].down_k, rep->level[1].down_k, rep->level[2].down_k};
    const int32_t up_k[3] = {rep->level[0].up_k, rep->level[1].up_k, rep->level[2].up_k};
    return write_thr_line(path, down_k, up_k, order, "ethcnn_calib_write_thr_info");
}
