// ethcnn_ldp_group.cpp -- config #5 offline, group form (include/ethcnn.h): K residual sequences of one geometry, each with its own
// ETH-LSTM bundle, QP, state and output, through ONE recurrence launch per run of frames.  Member m's result is what
// ethcnn_ldp_sequence_device gives on a context that holds m's bundle, bit for bit: that call is a group of one through the same
// front-end (seq_front, per member), run loop (seq_recur) and kernels (ethcnn_lstm_seq.hip).
#include "ethcnn_ctx.h"
#include "ethcnn_ldp_group.h"

namespace {
int gerr(ethcnn_ldp_group* g, int code, const char* fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g->err = buf;
    return code;
}
#define GCHK(g, call)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return gerr((g), ETHCNN_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

constexpr int64_t kStateFloats = 2 * kNVec;  // (c, h) of a CTU

int check_member(ethcnn_ldp_group* g, int m, const char* who) {
    if (m < 0 || m >= g->k) return gerr(g, ETHCNN_ERR_ARG, "%s: member %d outside 0..%d", who, m, g->k - 1);
    return 0;
}

int upload_member(ethcnn_ldp_group* g, int m) {
    ethcnn_ldp_group::Member& M = g->m[m];
    const int rc = upload_lstm_image(g->c, M.blob.data(), &M.d_lstm);
    if (rc) {
        M.have = false;  // (the image may be half written)
        return gerr(g, rc, "member %d: %s", m, g->c->err.c_str());
    }
    M.have = true;
    return ETHCNN_OK;
}
}  // namespace

extern "C" int64_t ethcnn_ldp_group_bytes(int w, int h, int nframes, int chunk_frames, int k) {
    if (w <= 0 || h <= 0 || nframes <= 0 || chunk_frames < 0 || k < 1 || k > kLstmSeqGroupMax) return ETHCNN_ERR_ARG;
    const int64_t nctu = (int64_t)((w + 63) / 64) * ((h + 63) / 64), cap = (nctu + 15) / 16 * 16;
    const int64_t F = seq_chunk_frames(nctu, nframes, chunk_frames, k);
    return k * F * nctu * kNVec * 4 + k * cap * kStateFloats * 4;
}

extern "C" int ethcnn_ldp_group_create(ethcnn_ctx* c, int k, ethcnn_ldp_group** out) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "null output pointer");
    *out = nullptr;
    if (k < 1 || k > kLstmSeqGroupMax) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_group_create: %d members (1..%d)", k, kLstmSeqGroupMax);
    ethcnn_ldp_group* g = new (std::nothrow) ethcnn_ldp_group;
    if (!g) return set_err(c, ETHCNN_ERR_NOMEM, "out of memory");
    g->c = c;
    g->k = k;
    *out = g;
    return ETHCNN_OK;
}

extern "C" void ethcnn_ldp_group_destroy(ethcnn_ldp_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->c->device);
    (void)hipStreamSynchronize(g->c->stream);
    for (int m = 0; m < g->k; ++m)
        if (g->m[m].d_lstm) (void)hipFree(g->m[m].d_lstm);
    if (g->d_vec) (void)hipFree(g->d_vec);
    if (g->d_state) (void)hipFree(g->d_state);
    delete g;
}

extern "C" const char* ethcnn_ldp_group_last_error(const ethcnn_ldp_group* g) { return g ? g->err.c_str() : "LDP group is NULL"; }
extern "C" int ethcnn_ldp_group_count(const ethcnn_ldp_group* g) { return g ? g->k : ETHCNN_ERR_ARG; }

extern "C" int ethcnn_ldp_group_load_lstm_blob(ethcnn_ldp_group* g, int m, const float* blob, size_t nfloats) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = check_member(g, m, "ethcnn_ldp_group_load_lstm_blob")) return rc;
    if (!blob) return gerr(g, ETHCNN_ERR_ARG, "null pointer");
    if (nfloats != kLstmBlobFloats) return gerr(g, ETHCNN_ERR_ARG, "LSTM blob must hold %zu floats, got %zu", (size_t)kLstmBlobFloats, nfloats);
    g->m[m].blob.assign(blob, blob + nfloats);
    return upload_member(g, m);
}

extern "C" int ethcnn_ldp_group_load_lstm_synthetic(ethcnn_ldp_group* g, int m, uint64_t seed, double head_gain) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = check_member(g, m, "ethcnn_ldp_group_load_lstm_synthetic")) return rc;
    g->m[m].blob.resize(kLstmBlobFloats);
    synth_lstm_blob(seed, head_gain, g->m[m].blob.data());
    return upload_member(g, m);
}

extern "C" int ethcnn_ldp_group_load_lstm_checkpoint(ethcnn_ldp_group* g, int m, const char* prefix) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = check_member(g, m, "ethcnn_ldp_group_load_lstm_checkpoint")) return rc;
    if (!prefix) return gerr(g, ETHCNN_ERR_ARG, "null pointer");
    std::vector<float> blob(kLstmBlobFloats);
    char err[400];
    const int rc = ckpt_load_table(prefix, kLstmTensors, kNumLstmTensors, blob.data(), err, sizeof err);
    if (rc) return gerr(g, rc, "member %d: %s", m, err);  // (the member keeps the bundle it had)
    g->m[m].blob.swap(blob);
    return upload_member(g, m);
}

extern "C" int ethcnn_ldp_group_get_lstm_blob(ethcnn_ldp_group* g, int m, float* out, size_t nfloats) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = check_member(g, m, "ethcnn_ldp_group_get_lstm_blob")) return rc;
    if (!out || nfloats != kLstmBlobFloats) return gerr(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_get_lstm_blob: a buffer of %zu floats", (size_t)kLstmBlobFloats);
    if (!g->m[m].have) return gerr(g, ETHCNN_ERR_NOWEIGHTS, "member %d has no ETH-LSTM bundle loaded", m);
    std::memcpy(out, g->m[m].blob.data(), nfloats * 4);
    return ETHCNN_OK;
}

extern "C" int ethcnn_ldp_group_set_chunk(ethcnn_ldp_group* g, int frames) {
    if (!g) return ETHCNN_ERR_ARG;
    if (frames < 0) return gerr(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_set_chunk: %d frames", frames);
    g->chunk = frames;
    return ETHCNN_OK;
}

extern "C" int64_t ethcnn_ldp_group_state_ctus(ethcnn_ldp_group* g, int m) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = check_member(g, m, "ethcnn_ldp_group_state_ctus")) return rc;
    return g->m[m].state_nctu < 0 ? 0 : g->m[m].state_nctu;
}

extern "C" int ethcnn_ldp_group_get_state(ethcnn_ldp_group* g, int m, float* out, size_t nfloats) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = check_member(g, m, "ethcnn_ldp_group_get_state")) return rc;
    if (!out) return gerr(g, ETHCNN_ERR_ARG, "null pointer");
    const ethcnn_ldp_group::Member& M = g->m[m];
    if (M.state_nctu < 0) return gerr(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_get_state: member %d has no resident state", m);
    if (nfloats != (size_t)M.state_nctu * kStateFloats)
        return gerr(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_get_state: the resident state of member %d holds %zu floats, not %zu", m,
                    (size_t)M.state_nctu * kStateFloats, nfloats);
    ethcnn_ctx* c = g->c;
    GCHK(g, hipSetDevice(c->device));
    GCHK(g, hipMemcpyAsync(out, g->d_state + (size_t)m * g->state_cap * kStateFloats, nfloats * 4, hipMemcpyDeviceToHost, c->stream));
    GCHK(g, hipStreamSynchronize(c->stream));
    return ETHCNN_OK;
}

extern "C" int ethcnn_ldp_group_sequence_device(ethcnn_ldp_group* g, const uint8_t* const* d_luma, int w, int h, ptrdiff_t pitch, ptrdiff_t fstride,
                                                int nframes, const int* qp, int i_first, const float* const* d_state_in, float* const* d_probs) {
    if (!g) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = g->c;
    const int K = g->k;
    // ---- checks: nothing is allocated or enqueued before they pass
    if (c->ldp.open || c->ai.open) return gerr(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_sequence: a streamed call has not been ended");
    if (!c->have_weights) return gerr(g, ETHCNN_ERR_NOWEIGHTS, "no CNN weights loaded");
    for (int m = 0; m < K; ++m)
        if (!g->m[m].have) return gerr(g, ETHCNN_ERR_NOWEIGHTS, "member %d has no ETH-LSTM bundle loaded (ethcnn_ldp_group_load_lstm_*)", m);
    if (!d_luma || !qp || !d_probs) return gerr(g, ETHCNN_ERR_ARG, "null pointer");
    for (int m = 0; m < K; ++m)
        if (!d_luma[m] || !d_probs[m]) return gerr(g, ETHCNN_ERR_ARG, "null pointer (member %d)", m);
    for (int m = 0; m < K; ++m) {  // lstm_seq_level reads a state as float4; d_probs is touched dword by dword
        if (d_state_in && (uintptr_t)d_state_in[m] % 16) return gerr(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_sequence: d_state_in[%d] is not 16-byte aligned", m);
        if ((uintptr_t)d_probs[m] % 4) return gerr(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_sequence: d_probs[%d] is not 4-byte aligned", m);
    }
    if (w <= 0 || h <= 0 || pitch < w) return gerr(g, ETHCNN_ERR_ARG, "bad geometry");
    if (nframes <= 0) return gerr(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_sequence: nframes must be positive");
    if (i_first < 0) return gerr(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_sequence: i_frame_first must not be negative");
    const int nctu = ((w + 63) / 64) * ((h + 63) / 64);
    if (i_first > 1)
        for (int m = 0; m < K; ++m)
            if (!(d_state_in && d_state_in[m]) && g->m[m].state_nctu != nctu)
                return gerr(g, ETHCNN_ERR_ARG, "ethcnn_ldp_step: frame %d needs the previous frame's state, but none is resident for %d CTUs (member %d)",
                            i_first, nctu, m);
    FrameGeom geom;
    if (int rc = make_geom(c, w, h, pitch, fstride, &geom)) return gerr(g, rc, "%s", c->err.c_str());
    // ---- buffers: refused with the whole sum before anything is allocated
    const int64_t F = seq_chunk_frames(nctu, nframes, g->chunk, K);
    const int cap = (nctu + 15) / 16 * 16;
    const size_t slice = (size_t)F * nctu * kNVec, vb = (size_t)K * slice * 4, sb = (size_t)K * cap * kStateFloats * 4;
    GCHK(g, hipSetDevice(c->device));
    size_t grow = 0, back = 0;
    if (vb > g->vec_cap) grow += vb, back += g->vec_cap;
    if (cap > g->state_cap) grow += sb, back += (size_t)K * g->state_cap * kStateFloats * 4;
    if (grow) {
        size_t free_b = 0, total_b = 0;
        GCHK(g, hipMemGetInfo(&free_b, &total_b));
        if (grow > free_b + back)
            return gerr(g, ETHCNN_ERR_NOMEM, "ethcnn_ldp_group_sequence: %d members in chunks of %lld frames hold %lld bytes on the device (ethcnn_ldp_group_bytes); %zu are free",
                        K, (long long)F, (long long)ethcnn_ldp_group_bytes(w, h, (int)F, (int)F, K), free_b + back);
        GCHK(g, hipStreamSynchronize(c->stream));
        if (!seq_grow(&g->d_vec, &g->vec_cap, vb)) return gerr(g, ETHCNN_ERR_NOMEM, "ethcnn_ldp_group_sequence: %zu bytes of vectors do not fit", vb);
        if (cap > g->state_cap) {  // (no member continues from a resident state then: it would belong to a smaller CTU count)
            size_t held = 0;  // (state_cap counts CTUs per member, not bytes)
            g->state_cap = 0;
            for (int m = 0; m < K; ++m) g->m[m].state_nctu = -1;
            if (!seq_grow(&g->d_state, &held, sb)) return gerr(g, ETHCNN_ERR_NOMEM, "ethcnn_ldp_group_sequence: %zu bytes of states do not fit", sb);
            g->state_cap = cap;
        }
    }
    // ---- the chunk loop.  A member's resident state is advanced in place: a block stores only its own columns (ethcnn_lstm_seq.h)
    c->done_armed = 0;
    const float* sin[kLstmSeqGroupMax];
    const float* vec[kLstmSeqGroupMax];
    const float* lstm[kLstmSeqGroupMax];
    float* sout[kLstmSeqGroupMax];
    for (int m = 0; m < K; ++m) {
        vec[m] = g->d_vec + (size_t)m * slice;
        lstm[m] = g->m[m].d_lstm;
        sout[m] = g->d_state + (size_t)m * g->state_cap * kStateFloats;
        sin[m] = i_first > 1 ? ((d_state_in && d_state_in[m]) ? d_state_in[m] : sout[m]) : nullptr;
        g->m[m].state_nctu = -1;  // until every frame has been enqueued
    }
    for (int64_t f0 = 0; f0 < nframes; f0 += F) {
        const int nf = (int)std::min<int64_t>(F, nframes - f0);
        for (int m = 0; m < K; ++m)
            if (int rc = seq_front(c, d_luma[m] + f0 * fstride, geom, nf, g->d_vec + (size_t)m * slice))
                return gerr(g, rc, "member %d: %s (the resident states of the group were dropped)", m, c->err.c_str());
        float* probs[kLstmSeqGroupMax];
        for (int m = 0; m < K; ++m) probs[m] = d_probs[m] + (size_t)f0 * nctu * kNOut;
        const hipError_t e = seq_recur(c, K, vec, sin, sout, lstm, qp, probs, nctu, nf, i_first + (int)f0);
        if (e != hipSuccess) return gerr(g, ETHCNN_ERR_DEVICE, "launch failed: %s (the resident states of the group were dropped)", hipGetErrorString(e));
    }
    for (int m = 0; m < K; ++m) g->m[m].state_nctu = nctu;
    return serial_end(c);
}
