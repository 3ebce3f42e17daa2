// ethcnn_pacer.cpp -- host side of the online search budget (include/ethcnn.h "search budget, online"): the pacer object around
// k_pacer_frame (ethcnn_pacer.hip) and k_budget_bake (ethcnn_budget.hip), two launches a frame on the context's stream.
#include "ethcnn_analysis.h"
#include "ethcnn_budget.h"
#include "ethcnn_pacer.h"

using namespace ethcnn::pacer;
using ethcnn::budget::kDefaultRungs;
using ethcnn::budget::kMaxFrameCtus;
using ethcnn::budget::kNout;

struct ethcnn_pacer {
    ethcnn_ctx* c = nullptr;
    int64_t K = 0;
    uint64_t weight[4] = {};  // (set by ethcnn_pacer_create)
    uint32_t budget_ppm = 0;
    int mode = 0;
    int* d_thr = nullptr;          // [K + 1][6]: the ladder, then the full search
    unsigned* d_checked = nullptr; // [K + 1][4]
    unsigned* d_state = nullptr;   // [kStateWords]
    unsigned* d_recs = nullptr;    // record scratch, 64 bytes a CTU
    int64_t cap_recs = 0;          // in CTUs
    float* d_stage = nullptr;      // staging of the host form for pageable pointers, 84 bytes a CTU
    int64_t cap_stage = 0;
    ethcnn_pacer_result* h_result = nullptr;  // page-locked
    int64_t queued = 0;            // frames enqueued since create / reset
};

namespace ethcnn {
namespace pacer {
int check_rules(ethcnn_ctx* c, const ethcnn_sim_thr* ladder, int64_t K, const uint64_t* weight, uint32_t budget_ppm, int mode) {
    if (ladder) {
        if (int rc = sim::check_rung_count(c, K)) return rc;
        for (int64_t i = 0; i < K; ++i)
            if (int rc = sim::check_cand(c, ladder[i], (long long)i)) return rc;
    }
    if (int rc = sim::check_weights(c, weight)) return rc;
    if (budget_ppm > 1000000u) return set_err(c, ETHCNN_ERR_ARG, "the budget is in parts per million, 0..1000000: got %u", budget_ppm);
    if (mode != ETHCNN_BUDGET_FRAME && mode != ETHCNN_BUDGET_CARRY)
        return set_err(c, ETHCNN_ERR_ARG, "mode %d is neither ETHCNN_BUDGET_FRAME nor ETHCNN_BUDGET_CARRY", mode);
    return 0;
}

int check_frame(ethcnn_ctx* c, const uint64_t weight[4], int width, int height, int64_t* per) {
    sim::PicSize s;
    if (int rc = sim::check_size(c, width, height, 8, &s)) return rc;
    *per = s.ctus();
    if (*per >= kMaxFrameCtus) return set_err(c, ETHCNN_ERR_ARG, "a frame of %lld CTUs does not count in 32 bits (fewer than 2^24)", (long long)*per);
    if (!sim::cost_fits(*per, weight)) return set_err(c, ETHCNN_ERR_ARG, "the cost of a frame of %lld CTUs may not fit in 64 bits under these weights", (long long)*per);
    return 0;
}

int grow(ethcnn_ctx* c, void** buf, int64_t* cap, int64_t want, int64_t bytes_each, const char* what) {
    if (want <= *cap) return 0;
    void* d = nullptr;
    if (hipMalloc(&d, (size_t)(want * bytes_each)) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, ETHCNN_ERR_NOMEM, "search budget, online: %lld bytes of %s for %lld CTUs do not fit in device memory", (long long)(want * bytes_each), what,
                       (long long)want);
    }
    if (*buf) {
        HIPCHK(c, hipStreamSynchronize(c->stream));  // an earlier frame may still use the old one
        (void)hipFree(*buf);
    }
    *buf = d;
    *cap = want;
    return 0;
}

std::vector<int> ladder_rows(const ethcnn_sim_thr* ladder, int64_t K) {
    std::vector<ethcnn_sim_thr> lad;
    if (ladder) lad.assign(ladder, ladder + K);
    else {
        lad.resize(kDefaultRungs);
        ethcnn_budget_default_ladder(lad.data());
    }
    lad.push_back(sim::kFullSearch);  // rung K
    std::vector<int> rows;
    for (const ethcnn_sim_thr& t : lad) {
        for (int l = 0; l < 3; ++l) rows.push_back(t.up_k[l]);
        for (int l = 0; l < 3; ++l) rows.push_back(t.down_k[l]);
    }
    return rows;
}
}  // namespace pacer
}  // namespace ethcnn

namespace {
// checked arguments, device-addressable pointers: the two launches
int enqueue(ethcnn_pacer* p, const float* d_probs, int width, int height, int64_t per, float* d_baked, ethcnn_pacer_result* d_result) {
    ethcnn_ctx* c = p->c;
    c->done_armed = 0;  // the context's completion word does not cover these launches
    FrameArgs a;
    a.probs = d_probs;
    a.width = width, a.height = height, a.ctus_w = (width + 63) / 64;
    a.per = (int)per;
    a.thr = p->d_thr;
    a.rungs = (int)(p->K + 1);
    a.checked = p->d_checked;
    a.state = p->d_state;
    a.recs = p->d_recs;
    for (int d = 0; d < 4; ++d) a.weight[d] = p->weight[d];
    a.budget_ppm = p->budget_ppm;
    a.carry_mode = p->mode == ETHCNN_BUDGET_CARRY;
    a.d_result = d_result;
    a.h_result = p->h_result;
    (void)hipGetLastError();
    launch_frame(c->stream, a);
    ethcnn::budget::launch_bake(c->stream, p->d_recs, (long)per, 0, (long)per, reinterpret_cast<const int*>(p->d_state + kStateThr), d_baked);
    HIPCHK(c, hipGetLastError());
    ++p->queued;
    return 0;
}

int check_call(ethcnn_pacer* p, const void* probs, const void* baked, int width, int height, int64_t* per) {
    if (int rc = check_frame(p->c, p->weight, width, height, per)) return rc;
    if (!probs || !baked) return set_err(p->c, ETHCNN_ERR_ARG, "null probabilities or output buffer");
    return 0;
}
}  // namespace

extern "C" int ethcnn_pacer_check(const ethcnn_sim_thr* ladder, int64_t K, const uint64_t weight[4], uint32_t budget_ppm, int mode) {
    return check_rules(nullptr, ladder, K, weight, budget_ppm, mode);
}

extern "C" int ethcnn_pacer_create(ethcnn_ctx* c, const ethcnn_sim_thr* ladder, int64_t K, const uint64_t weight[4], uint32_t budget_ppm, int mode,
                                   ethcnn_pacer** out) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_create: null output");
    if (int rc = check_rules(c, ladder, K, weight, budget_ppm, mode)) return rc;
    const std::vector<int> rows = ladder_rows(ladder, K);
    HIPCHK(c, hipSetDevice(c->device));
    ethcnn_pacer* p = new ethcnn_pacer;
    p->c = c;
    p->K = (int64_t)rows.size() / 6 - 1;
    for (int d = 0; d < 4; ++d) p->weight[d] = (weight ? weight : sim::kDefaultWeight)[d];
    p->budget_ppm = budget_ppm;
    p->mode = mode;
    const size_t n = rows.size() / 6;
    hipError_t e = hipMalloc((void**)&p->d_thr, n * 24);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_checked, n * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_state, kStateWords * 4);
    if (e == hipSuccess) e = hipHostMalloc((void**)&p->h_result, sizeof(ethcnn_pacer_result), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_thr, rows.data(), n * 24, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_checked, 0, n * 16, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_state, 0, kStateWords * 4, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (rows is a temporary)
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ethcnn_pacer_destroy(p);
        return set_err(c, e == hipErrorOutOfMemory ? ETHCNN_ERR_NOMEM : ETHCNN_ERR_DEVICE, "ethcnn_pacer_create: %s (%llu bytes of tables)", hipGetErrorString(e),
                       (unsigned long long)(n * 40 + kStateWords * 4));
    }
    std::memset(p->h_result, 0, sizeof *p->h_result);
    *out = p;
    return ETHCNN_OK;
}

extern "C" void ethcnn_pacer_destroy(ethcnn_pacer* p) {
    if (!p) return;
    if (p->c && p->c->stream) (void)hipStreamSynchronize(p->c->stream);
    if (p->d_thr) (void)hipFree(p->d_thr);
    if (p->d_checked) (void)hipFree(p->d_checked);
    if (p->d_state) (void)hipFree(p->d_state);
    if (p->d_recs) (void)hipFree(p->d_recs);
    if (p->d_stage) (void)hipFree(p->d_stage);
    if (p->h_result) (void)hipHostFree(p->h_result);
    delete p;
}

extern "C" int ethcnn_pacer_reset(ethcnn_pacer* p) {
    if (!p) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = p->c;
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;
    // stream-ordered behind the frames already queued; table and ticket are zero between frames anyway
    HIPCHK(c, hipMemsetAsync(p->d_state, 0, kStateWords * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(p->d_checked, 0, (size_t)(p->K + 1) * 16, c->stream));
    p->queued = 0;
    return ETHCNN_OK;
}

extern "C" int ethcnn_pacer_frame_device(ethcnn_pacer* p, const float* d_probs, int width, int height, float* d_baked, ethcnn_pacer_result* d_result) {
    if (!p) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = p->c;
    int64_t per = 0;
    if (int rc = check_call(p, d_probs, d_baked, width, height, &per)) return rc;
    if ((uintptr_t)d_probs % 4 || (uintptr_t)d_baked % 4 || (uintptr_t)d_result % 4) return set_err(c, ETHCNN_ERR_ARG, "a device pointer is not 4-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = grow(c, (void**)&p->d_recs, &p->cap_recs, per, 64, "record scratch")) return rc;
    return enqueue(p, d_probs, width, height, per, d_baked, d_result);
}

extern "C" int ethcnn_pacer_frame(ethcnn_pacer* p, const float* probs, int width, int height, float* baked, ethcnn_pacer_result* result) {
    if (!p) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = p->c;
    int64_t per = 0;
    if (int rc = check_call(p, probs, baked, width, height, &per)) return rc;
    if ((uintptr_t)probs % 4 || (uintptr_t)baked % 4) return set_err(c, ETHCNN_ERR_ARG, "a pointer is not 4-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)per * kNout * 4;
    // a pointer inside an ethcnn_host_alloc buffer is read / written in place by the kernels; anything else goes through the staging
    const bool in_direct = in_pinned(c, probs, bytes), out_direct = in_pinned(c, baked, bytes);
    if (int rc = grow(c, (void**)&p->d_recs, &p->cap_recs, per, 64, "record scratch")) return rc;
    if (!in_direct || !out_direct)
        if (int rc = grow(c, (void**)&p->d_stage, &p->cap_stage, per, kNout * 4, "staging")) return rc;
    c->done_armed = 0;
    if (!in_direct) HIPCHK(c, hipMemcpyAsync(p->d_stage, probs, bytes, hipMemcpyHostToDevice, c->stream));
    if (int rc = enqueue(p, in_direct ? probs : p->d_stage, width, height, per, out_direct ? baked : p->d_stage, nullptr)) return rc;
    if (!out_direct) {
        HIPCHK(c, hipMemcpyAsync(baked, p->d_stage, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        // the wait: a bounded spin on the completion word that one lane stores behind the bake, hipStreamSynchronize as the fallback
        const unsigned seq = done_arm(c);
        if (seq) {
            launch_done(c->stream, c->h_done, seq);
            HIPCHK(c, hipGetLastError());
            c->done_armed = seq;
        }
        HIPCHK(c, stream_sync(c));
    }
    if (result) *result = *p->h_result;
    return ETHCNN_OK;
}

extern "C" int ethcnn_pacer_last(ethcnn_pacer* p, ethcnn_pacer_result* out) {
    if (!p) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = p->c;
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_last: null output");
    if (p->queued == 0) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_last: no frame has been paced since create / reset");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_sync(c));
    *out = *p->h_result;
    return ETHCNN_OK;
}
