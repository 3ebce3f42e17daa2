// ethcnn_audit.cpp -- host side of include/ethcnn.h "comparing two predictions": the four compare entries around the kernel of
// ethcnn_audit.hip, and the plan audit built on them (two runs of ethcnn_predict_luma_device over the caller's frames, plan 0 and the
// audited plan, compared in the frame layout).
#include <fcntl.h>

#include "ethcnn_analysis.h"
#include "ethcnn_audit.h"

using namespace ethcnn::audit;
using ethcnn::sim::kStageCtus;

namespace {
constexpr int kRow = kNOut * 4;  // bytes of a CTU's probabilities

void zero_stats(ethcnn_compare_stats* s) {
    std::memset(s, 0, sizeof *s);
    for (int l = 0; l < 3; ++l) s->worst_ctu[l] = -1;
}

// the rules every entry shares; *g is the launch geometry (per-CTU layout: width == 0), *n the CTU count
int check_rules(ethcnn_ctx* c, int width, int height, int64_t units, bool frames, float tol, const ethcnn_sim_thr* thr, Geom* g, int64_t* n) {
    if (units < 0) return set_err(c, ETHCNN_ERR_ARG, "compare: negative %s count %lld", frames ? "frame" : "CTU", (long long)units);
    if (!(tol >= 0.0f)) return set_err(c, ETHCNN_ERR_ARG, "compare: the tolerance must be a number >= 0");
    if (thr)
        if (int rc = ethcnn::sim::check_cand(c, *thr, 0)) return rc;
    *g = Geom{0, 0, 64, 64};
    int64_t per = 1;
    if (frames) {
        ethcnn::sim::PicSize s;
        if (int rc = ethcnn::sim::check_size(c, width, height, 8, &s)) return rc;
        *g = Geom{s.ctus_w, s.ctus_h, width, height};
        per = s.ctus();
    }
    if (units > (((int64_t)1 << 31) - 1) / per) return set_err(c, ETHCNN_ERR_ARG, "compare: 2^31 CTUs or more in one call");
    *n = units * per;
    return 0;
}

int check_args(ethcnn_ctx* c, const void* a, const void* b, int width, int height, int64_t units, bool frames, float tol, const ethcnn_sim_thr* thr,
               ethcnn_compare_stats* out, Geom* g, int64_t* n) {
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "compare: null output");
    if (int rc = check_rules(c, width, height, units, frames, tol, thr, g, n)) return rc;
    if (*n && (!a || !b)) return set_err(c, ETHCNN_ERR_ARG, "compare: null buffer");
    if (((uintptr_t)a | (uintptr_t)b) % 4) return set_err(c, ETHCNN_ERR_ARG, "compare: a buffer is not 4-byte aligned");
    return 0;
}

// what the audit's passes (and a guard that has to measure) change and the caller must find as it was
struct Saved {
    ethcnn_ctx* c;
    int plan, profiling, last_n, last_parity, last_fast;
    float thr1, thr2;
    unsigned fc1_sample;
    unsigned long passes;
    ethcnn_stage_times times;
    explicit Saved(ethcnn_ctx* c_)
        : c(c_), plan(c_->fc1_plan), profiling(c_->profiling), last_n(c_->last_n), last_parity(c_->last_parity), last_fast(c_->last_fast),
          thr1(c_->thr1), thr2(c_->thr2), fc1_sample(c_->fc1_sample), passes(c_->passes), times(c_->times) {}
    void restore() const {
        c->fc1_plan = plan;
        c->profiling = profiling;
        c->last_n = last_n;
        c->last_parity = last_parity;
        c->last_fast = last_fast;
        c->thr1 = thr1;
        c->thr2 = thr2;
        c->fc1_sample = fc1_sample;
        c->times = times;
        // the bookkeeping is the caller's again, the workspace is not: ethcnn_debug_fetch refuses until the next pass of the caller's
        if (c->passes != passes) c->ws_foreign = true;
    }
};

Thr thr_of(const ethcnn_sim_thr* thr) {
    Thr t{};
    if (thr) {
        for (int l = 0; l < 3; ++l) {
            t.up[l] = thr->up_k[l];
            t.down[l] = thr->down_k[l];
        }
        t.has_thr = 1;
    }
    return t;
}

int begin_call(ethcnn_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;  // the context's completion word does not cover these launches
    if (!c->d_compare) HIPCHK(c, hipMalloc((void**)&c->d_compare, kWords * 8));
    HIPCHK(c, hipMemsetAsync(c->d_compare, 0, kWords * 8, c->stream));
    return 0;
}

// waits for the launches of the call and turns its words into the result
int end_call(ethcnn_ctx* c, int64_t n, bool has_thr, ethcnn_compare_stats* out) {
    unsigned long long w[kWords];
    hipError_t e = hipMemcpyAsync(w, c->d_compare, sizeof w, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, ETHCNN_ERR_DEVICE, "compare: %s", hipGetErrorString(e));
    }
    zero_stats(out);
    out->ctus = (uint64_t)n;
    out->rejected_ctus = w[kRejected];
    for (int l = 0; l < 3; ++l) {
        out->over_tol[l] = w[kOverTol + l];
        out->bits_diff[l] = w[kBitsDiff + l];
        out->class_diff[l] = w[kClassDiff + l];
        if (w[kMax + l]) {
            const uint32_t bits = (uint32_t)(w[kMax + l] >> 32);
            std::memcpy(&out->max_abs[l], &bits, 4);
            out->worst_ctu[l] = (int64_t)(uint32_t)~(uint32_t)w[kMax + l];
        }
    }
    out->search_diff_ctus = w[kSearchDiff];
    for (int d = 0; d < 4; ++d) {
        out->checked_a[d] = w[kCheckedA + d];
        out->checked_b[d] = w[kCheckedB + d];
    }
    out->with_thr = has_thr ? 1u : 0u;
    return ETHCNN_OK;
}

int compare_device(ethcnn_ctx* c, const float* d_a, const float* d_b, int64_t n, const Geom& g, float tol, const ethcnn_sim_thr* thr,
                   ethcnn_compare_stats* out, uint8_t* d_flags) {
    if (n == 0) {
        zero_stats(out);
        out->with_thr = thr ? 1u : 0u;
        return ETHCNN_OK;
    }
    if (int rc = begin_call(c)) return rc;
    launch_compare(c->stream, d_a, d_b, (long)n, 0, g, tol, thr_of(thr), c->d_compare, d_flags, cus_of(c));
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return set_err(c, ETHCNN_ERR_DEVICE, "launch of the comparison failed: %s", hipGetErrorString(le));
    return end_call(c, n, thr != nullptr, out);
}

// host pointers: a pointer whose whole range lies in an ethcnn_host_alloc buffer is used in place, anything else goes through a device
// buffer in pieces of kStageCtus CTUs.  The pieces add into one call state with their global indices, so the result does not depend on them.
int compare_host(ethcnn_ctx* c, const float* a, const float* b, int64_t n, const Geom& g, float tol, const ethcnn_sim_thr* thr,
                 ethcnn_compare_stats* out, uint8_t* flags) {
    if (n == 0) return compare_device(c, a, b, 0, g, tol, thr, out, nullptr);
    const bool a_direct = in_pinned(c, a, (size_t)n * kRow), b_direct = in_pinned(c, b, (size_t)n * kRow);
    const bool f_direct = !flags || in_pinned(c, flags, (size_t)n);
    const int64_t piece = (a_direct && b_direct && f_direct) ? n : std::min(n, kStageCtus);
    const size_t bytes = (size_t)piece * ((a_direct ? 0 : kRow) + (b_direct ? 0 : kRow) + (f_direct ? 0 : 1));
    if (int rc = begin_call(c)) return rc;
    Scratch stage;
    if (bytes)
        if (int rc = stage.alloc(c, bytes, "compare", true)) return rc;
    float* d_a = stage.at<float>();
    float* d_b = stage.at<float>(a_direct ? 0 : (size_t)piece * kRow);
    uint8_t* d_f = stage.at((size_t)piece * ((a_direct ? 0 : kRow) + (b_direct ? 0 : kRow)));
    hipError_t e = hipSuccess;
    for (int64_t at = 0; at < n && e == hipSuccess; at += piece) {
        const int64_t m = std::min(piece, n - at);
        if (!a_direct) e = hipMemcpyAsync(d_a, a + at * kNOut, (size_t)m * kRow, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && !b_direct) e = hipMemcpyAsync(d_b, b + at * kNOut, (size_t)m * kRow, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) break;
        launch_compare(c->stream, a_direct ? a + at * kNOut : d_a, b_direct ? b + at * kNOut : d_b, (long)m, (long)at, g, tol, thr_of(thr), c->d_compare,
                       !flags ? nullptr : f_direct ? flags + at : d_f, cus_of(c));
        e = hipGetLastError();
        if (e == hipSuccess && flags && !f_direct) e = hipMemcpyAsync(flags + at, d_f, (size_t)m, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && piece < n) e = hipStreamSynchronize(c->stream);  // the next piece overwrites the staging
    }
    int rc = e == hipSuccess ? end_call(c, n, thr != nullptr, out) : set_err(c, ETHCNN_ERR_DEVICE, "compare: %s", hipGetErrorString(e));
    if (e != hipSuccess) (void)hipStreamSynchronize(c->stream);
    return rc;
}
}  // namespace

extern "C" int ethcnn_compare_probs_device(ethcnn_ctx* c, const float* d_a, const float* d_b, int64_t n, float tol, const ethcnn_sim_thr* thr,
                                           ethcnn_compare_stats* out, uint8_t* d_flags) {
    if (!c) return ETHCNN_ERR_ARG;
    Geom g;
    int64_t total = 0;
    if (int rc = check_args(c, d_a, d_b, 0, 0, n, false, tol, thr, out, &g, &total)) return rc;
    return compare_device(c, d_a, d_b, total, g, tol, thr, out, d_flags);
}

extern "C" int ethcnn_compare_frames_device(ethcnn_ctx* c, const float* d_a, const float* d_b, int width, int height, int64_t nframes, float tol,
                                            const ethcnn_sim_thr* thr, ethcnn_compare_stats* out, uint8_t* d_flags) {
    if (!c) return ETHCNN_ERR_ARG;
    Geom g;
    int64_t total = 0;
    if (int rc = check_args(c, d_a, d_b, width, height, nframes, true, tol, thr, out, &g, &total)) return rc;
    return compare_device(c, d_a, d_b, total, g, tol, thr, out, d_flags);
}

extern "C" int ethcnn_compare_probs(ethcnn_ctx* c, const float* a, const float* b, int64_t n, float tol, const ethcnn_sim_thr* thr,
                                    ethcnn_compare_stats* out, uint8_t* flags) {
    if (!c) return ETHCNN_ERR_ARG;
    Geom g;
    int64_t total = 0;
    if (int rc = check_args(c, a, b, 0, 0, n, false, tol, thr, out, &g, &total)) return rc;
    return compare_host(c, a, b, total, g, tol, thr, out, flags);
}

extern "C" int ethcnn_compare_frames(ethcnn_ctx* c, const float* a, const float* b, int width, int height, int64_t nframes, float tol,
                                     const ethcnn_sim_thr* thr, ethcnn_compare_stats* out, uint8_t* flags) {
    if (!c) return ETHCNN_ERR_ARG;
    Geom g;
    int64_t total = 0;
    if (int rc = check_args(c, a, b, width, height, nframes, true, tol, thr, out, &g, &total)) return rc;
    return compare_host(c, a, b, total, g, tol, thr, out, flags);
}

// ------------------------------------------------------------------------------------------------------------------- the audit ---
extern "C" int64_t ethcnn_audit_plan_bytes(int width, int height, int nframes) {
    if (width <= 0 || height <= 0 || nframes < 0) return -1;
    const int64_t one = (int64_t)nframes * ((width + 63) / 64) * ((height + 63) / 64) * kRow;
    return (one + 15) / 16 * 16 + one;  // the second set starts 16-byte aligned: the comparison keeps its 16-byte loads
}

extern "C" int ethcnn_audit_plan_device(ethcnn_ctx* c, const uint8_t* d_luma, int width, int height, ptrdiff_t pitch, ptrdiff_t frame_stride, int nframes,
                                        int qp, int plan, float tol, const ethcnn_sim_thr* thr, ethcnn_audit_result* out) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!out || !d_luma || nframes < 0) return set_err(c, ETHCNN_ERR_ARG, "audit: null pointer / negative frame count");
    if (plan != 2 && plan != 3) return set_err(c, ETHCNN_ERR_ARG, "audit: plan must be 2 or 3, got %d", plan);
    if (c->ldp.open || c->ai.open) return set_err(c, ETHCNN_ERR_ARG, "audit: a streamed call has not been ended");
    if (!c->have_weights) return set_err(c, ETHCNN_ERR_NOWEIGHTS, "no weights loaded");
    Geom g;
    int64_t n = 0;
    if (int rc = check_rules(c, width, height, nframes, true, tol, thr, &g, &n)) return rc;
    FrameGeom fg;
    if (int rc = make_geom(c, width, height, pitch, frame_stride, &fg)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // the guard first: a refused plan changes nothing (its weight images are built here as well, outside the audited run)
    const Saved saved(c);
    c->profiling = 0;
    if (int rc = ensure_fast_weights(c, plan)) {
        saved.restore();
        return rc;
    }
    std::memset(out, 0, sizeof *out);
    zero_stats(&out->stats);
    out->stats.with_thr = thr ? 1u : 0u;
    out->plan = plan;
    if (nframes == 0) {
        saved.restore();
        return ETHCNN_OK;
    }
    const size_t bytes = (size_t)ethcnn_audit_plan_bytes(width, height, nframes);
    Scratch probs;  // the two sets of probabilities
    if (int rc = probs.alloc(c, bytes, "audit", true)) {
        saved.restore();
        return rc;
    }
    float* const d_p = probs.at<float>();
    c->thr1 = c->thr2 = -1.0f;  // gates open: a gate's knife edge is not an arithmetic error
    c->fc1_plan = 0;
    float* const d_q = d_p + ((size_t)n * kNOut + 3) / 4 * 4;  // side b, 16-byte aligned
    int rc = ethcnn_predict_luma_device(c, d_luma, width, height, pitch, frame_stride, nframes, qp, d_p);
    const unsigned long passes0 = c->passes, fast0 = c->fast_passes;
    if (rc == 0) {
        c->fc1_plan = plan;
        rc = ethcnn_predict_luma_device(c, d_luma, width, height, pitch, frame_stride, nframes, qp, d_q);
    }
    out->passes = (int32_t)(c->passes - passes0);
    out->fast_passes = (int32_t)(c->fast_passes - fast0);
    saved.restore();
    if (rc == 0) rc = compare_device(c, d_p, d_q, n, g, tol, thr, &out->stats, nullptr);
    else (void)hipStreamSynchronize(c->stream);
    return rc;
}

extern "C" int ethcnn_audit_plan_yuv_file(ethcnn_ctx* c, const char* path, int width, int height, int qp, int plan, int64_t first, int64_t step,
                                          int64_t count, float tol, const ethcnn_sim_thr* thr, ethcnn_audit_result* out) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!path || !out) return set_err(c, ETHCNN_ERR_ARG, "audit: null pointer");
    if (c->src_fmt.bit_depth != 8 || c->src_fmt.chroma_format != 420)
        return set_err(c, ETHCNN_ERR_ARG, "audit: the file entry reads 8-bit 4:2:0 only (the context's source format is %d-bit %d)", c->src_fmt.bit_depth,
                       c->src_fmt.chroma_format);
    if (plan != 2 && plan != 3) return set_err(c, ETHCNN_ERR_ARG, "audit: plan must be 2 or 3, got %d", plan);
    ethcnn::sim::PicSize size;
    if (int rc = ethcnn::sim::check_size(c, width, height, 8, &size)) return rc;
    if (first < 0 || step < 1 || count < 0 || count > 0x7fffffff) return set_err(c, ETHCNN_ERR_ARG, "audit: first >= 0, step >= 1 and count >= 0 are required");
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return set_err(c, ETHCNN_ERR_IO, "cannot open %s: %s", path, std::strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0) {
        close(fd);
        return set_err(c, ETHCNN_ERR_IO, "cannot examine %s: %s", path, std::strerror(errno));
    }
    const int64_t plane = (int64_t)width * height, fsz = plane * 3 / 2, frames = (int64_t)st.st_size / fsz;
    if (count > 0 && (first >= frames || (count - 1) > (frames - 1 - first) / step)) {
        close(fd);
        return set_err(c, ETHCNN_ERR_ARG, "audit: frame %lld lies past the end of %s (%lld frames of %d x %d)", (long long)(first + (count - 1) * step), path,
                       (long long)frames, width, height);
    }
    if (hipSetDevice(c->device) != hipSuccess) {
        close(fd);
        return set_err(c, ETHCNN_ERR_DEVICE, "hipSetDevice failed");
    }
    // the luma planes of the picked frames in one contiguous device buffer (at least one byte, so the pointer is never null)
    const size_t bytes = (size_t)std::max<int64_t>(count * plane, 1);
    size_t free_b = 0, total_b = 0;
    uint8_t* d_luma = nullptr;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes + (size_t)ethcnn_audit_plan_bytes(width, height, (int)count) > free_b ||
        hipMalloc((void**)&d_luma, bytes) != hipSuccess) {
        (void)hipGetLastError();
        close(fd);
        return set_err(c, ETHCNN_ERR_NOMEM, "audit: %llu bytes of luma and probabilities do not fit in device memory",
                       (unsigned long long)(bytes + (size_t)ethcnn_audit_plan_bytes(width, height, (int)count)));
    }
    int rc = 0;
    std::vector<uint8_t> host((size_t)plane);
    for (int64_t i = 0; i < count && rc == 0; ++i) {
        size_t got = 0;
        while (got < (size_t)plane) {
            const ssize_t r = pread(fd, host.data() + got, (size_t)plane - got, (off_t)((first + i * step) * fsz + (int64_t)got));
            if (r <= 0) {
                rc = set_err(c, ETHCNN_ERR_IO, "cannot read frame %lld of %s", (long long)(first + i * step), path);
                break;
            }
            got += (size_t)r;
        }
        if (rc == 0 && hipMemcpy(d_luma + i * plane, host.data(), (size_t)plane, hipMemcpyHostToDevice) != hipSuccess)
            rc = set_err(c, ETHCNN_ERR_DEVICE, "audit: the copy of frame %lld to the device failed", (long long)(first + i * step));
    }
    close(fd);
    if (rc == 0) rc = ethcnn_audit_plan_device(c, d_luma, width, height, width, (ptrdiff_t)plane, (int)count, qp, plan, tol, thr, out);
    (void)hipFree(d_luma);
    return rc;
}
