// ethcnn_ldp_set.cpp -- config #5 offline, group and batch form: the object both handles are (bundles, resident states, the vector
// buffer) and the run both device entries end in.  Sequence j's result is what ethcnn_ldp_sequence_device gives on a context that
// holds j's bundle, bit for bit: the same front-end (seq_front, per sequence), the same launch part (seq_launch) and the same kernel
// bodies (ethcnn_lstm_seq.hip), which take n, F and i_frame0 from the sequence's own row.
#include "ethcnn_ldp_set.h"

int ldp_set_err(LdpSet* s, int code, const char* fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    s->err = buf;
    return code;
}
#define SCHK(s, call)                                                                                         \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) return ldp_set_err((s), ETHCNN_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

namespace {
// i names a bundle, or (state) a resident state
int check_index(LdpSet* s, int i, bool state, const char* who, const char* what) {
    if (!s) return ETHCNN_ERR_ARG;
    const int count = state ? s->nstates : s->nb;
    if (i < 0 || i >= count) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: %s %d outside 0..%d", who, what, i, count - 1);
    return 0;
}

int upload(LdpSet* s, int i, const char* what) {
    LdpSet::Bundle& B = s->b[i];
    const int rc = upload_lstm_image(s->c, B.blob.data(), &B.d_lstm);
    if (rc) {
        B.have = false;  // (the image may be half written)
        return ldp_set_err(s, rc, "%s %d: %s", what, i, s->c->err.c_str());
    }
    B.have = true;
    return ETHCNN_OK;
}

void drop_states(LdpSet* s) {
    for (auto& S : s->s) S.state_nctu = -1;
}
}  // namespace

void ldp_set_release(LdpSet* s) {
    if (!s) return;
    (void)hipSetDevice(s->c->device);
    (void)hipStreamSynchronize(s->c->stream);
    for (auto& B : s->b)
        if (B.d_lstm) (void)hipFree(B.d_lstm);
    for (auto& S : s->s)
        if (S.d_state) (void)hipFree(S.d_state);
    if (s->d_vec) (void)hipFree(s->d_vec);
}

int ldp_set_load_blob(LdpSet* s, int i, const float* blob, size_t nfloats, const char* who, const char* what) {
    if (int rc = check_index(s, i, false, who, what)) return rc;
    if (!blob) return ldp_set_err(s, ETHCNN_ERR_ARG, "null pointer");
    if (nfloats != kLstmBlobFloats) return ldp_set_err(s, ETHCNN_ERR_ARG, "LSTM blob must hold %zu floats, got %zu", (size_t)kLstmBlobFloats, nfloats);
    s->b[i].blob.assign(blob, blob + nfloats);
    return upload(s, i, what);
}

int ldp_set_load_synthetic(LdpSet* s, int i, uint64_t seed, double head_gain, const char* who, const char* what) {
    if (int rc = check_index(s, i, false, who, what)) return rc;
    s->b[i].blob.resize(kLstmBlobFloats);
    synth_lstm_blob(seed, head_gain, s->b[i].blob.data());
    return upload(s, i, what);
}

int ldp_set_load_checkpoint(LdpSet* s, int i, const char* prefix, const char* who, const char* what) {
    if (int rc = check_index(s, i, false, who, what)) return rc;
    if (!prefix) return ldp_set_err(s, ETHCNN_ERR_ARG, "null pointer");
    std::vector<float> blob(kLstmBlobFloats);
    char err[400];
    const int rc = ckpt_load_table(prefix, kLstmTensors, kNumLstmTensors, blob.data(), err, sizeof err);
    if (rc) return ldp_set_err(s, rc, "%s %d: %s", what, i, err);  // (the index keeps the bundle it had)
    s->b[i].blob.swap(blob);
    return upload(s, i, what);
}

int ldp_set_get_blob(LdpSet* s, int i, float* out, size_t nfloats, const char* who, const char* what) {
    if (int rc = check_index(s, i, false, who, what)) return rc;
    if (!out || nfloats != kLstmBlobFloats) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: a buffer of %zu floats", who, (size_t)kLstmBlobFloats);
    if (!s->b[i].have) return ldp_set_err(s, ETHCNN_ERR_NOWEIGHTS, "%s %d has no ETH-LSTM bundle loaded", what, i);
    std::memcpy(out, s->b[i].blob.data(), nfloats * 4);
    return ETHCNN_OK;
}

int ldp_set_chunk(LdpSet* s, int frames, const char* who) {
    if (!s) return ETHCNN_ERR_ARG;
    if (frames < 0) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: %d frames", who, frames);
    s->chunk = frames;
    return ETHCNN_OK;
}

int64_t ldp_set_state_ctus(LdpSet* s, int j, const char* who, const char* what) {
    if (int rc = check_index(s, j, true, who, what)) return rc;
    return s->s[j].state_nctu < 0 ? 0 : s->s[j].state_nctu;
}

int ldp_set_get_state(LdpSet* s, int j, float* out, size_t nfloats, const char* who, const char* what) {
    if (int rc = check_index(s, j, true, who, what)) return rc;
    if (!out) return ldp_set_err(s, ETHCNN_ERR_ARG, "null pointer");
    const LdpSet::State& S = s->s[j];
    if (S.state_nctu < 0) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: %s %d has no resident state", who, what, j);
    if (nfloats != (size_t)S.state_nctu * kLdpStateFloats)
        return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: the resident state of %s %d holds %zu floats, not %zu", who, what, j,
                           (size_t)S.state_nctu * kLdpStateFloats, nfloats);
    ethcnn_ctx* c = s->c;
    SCHK(s, hipSetDevice(c->device));
    SCHK(s, hipMemcpyAsync(out, S.d_state, nfloats * 4, hipMemcpyDeviceToHost, c->stream));
    SCHK(s, hipStreamSynchronize(c->stream));
    return ETHCNN_OK;
}

namespace {
int check_gates_call(LdpSet* s, int j, const char* who, const char* what) {
    if (int rc = check_index(s, j, true, who, what)) return rc;
    if (s->c->ldp.open || s->c->ai.open) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: a streamed call has not been ended", who);
    return 0;
}
}  // namespace

int ldp_set_set_gates(LdpSet* s, int j, float thr1, float thr2, const char* who, const char* what) {
    if (int rc = check_gates_call(s, j, who, what)) return rc;
    LdpSet::State& S = s->s[j];
    S.own_gates = true;
    S.thr1 = thr1;
    S.thr2 = thr2;
    return ETHCNN_OK;
}

int ldp_set_clear_gates(LdpSet* s, int j, const char* who, const char* what) {
    if (int rc = check_gates_call(s, j, who, what)) return rc;
    s->s[j].own_gates = false;
    return ETHCNN_OK;
}

int ldp_set_get_gates(LdpSet* s, int j, float* thr1, float* thr2, int* own_out, const char* who, const char* what) {
    if (int rc = check_gates_call(s, j, who, what)) return rc;
    if (!thr1 || !thr2 || !own_out) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: null output pointer", who);
    ldp_set_gates_of(s, j, thr1, thr2);
    *own_out = s->s[j].own_gates ? 1 : 0;
    return ETHCNN_OK;
}

int ldp_set_run(LdpSet* s, const LdpSeq* seqs, int nseqs, const char* who, const char* item, const char* form) {
    ethcnn_ctx* c = s->c;
    // ---- buffers: refused with the whole sum before anything is allocated
    int64_t sum_nctu = 0, longest = 0;
    for (int j = 0; j < nseqs; ++j) sum_nctu += seqs[j].geom.nctu, longest = std::max<int64_t>(longest, seqs[j].nframes);
    const int64_t Fc = seq_chunk_frames(sum_nctu, s->chunk);
    const auto state_bytes = [](int64_t n) { return (size_t)((n + 15) / 16 * 16 * kLdpStateFloats * 4); };  // whole column groups
    size_t slice[kLstmSeqBatchMax + 1];  // sequence j's vectors start at float slice[j]
    slice[0] = 0;
    int64_t total = 0, front_ctus = 0;
    for (int j = 0; j < nseqs; ++j) {
        const int64_t n = seqs[j].geom.nctu, nf = std::min<int64_t>(seqs[j].nframes, Fc);
        slice[j + 1] = slice[j] + (size_t)(nf * n * kNVec);
        total += nf * n * kNVec * 4 + (int64_t)state_bytes(n);
        front_ctus = std::max<int64_t>(front_ctus, std::min<int64_t>(n * nf, c->max_ctus));
    }
    const size_t vb = slice[nseqs] * 4;
    SCHK(s, hipSetDevice(c->device));
    size_t grow = 0, back = 0;
    if (vb > s->vec_cap) grow += vb, back += s->vec_cap;
    for (int j = 0; j < nseqs; ++j)
        if (seqs[j].geom.nctu > s->s[j].cap) grow += state_bytes(seqs[j].geom.nctu), back += state_bytes(s->s[j].cap);
    if (grow) {
        size_t free_b = 0, total_b = 0;
        SCHK(s, hipMemGetInfo(&free_b, &total_b));
        if (grow > free_b + back)
            return ldp_set_err(s, ETHCNN_ERR_NOMEM, "%s: %d %ss in chunks of %lld frames hold %lld bytes on the device (ethcnn_ldp_%s_bytes); %zu are free",
                               who, nseqs, item, (long long)std::min(Fc, longest), (long long)total, form, free_b + back);
        SCHK(s, hipStreamSynchronize(c->stream));
        if (!seq_grow(&s->d_vec, &s->vec_cap, vb)) return ldp_set_err(s, ETHCNN_ERR_NOMEM, "%s: %zu bytes of vectors do not fit", who, vb);
        for (int j = 0; j < nseqs; ++j) {
            LdpSet::State& S = s->s[j];
            if (seqs[j].geom.nctu <= S.cap) continue;
            // (this index does not continue from its resident state: that belongs to a smaller CTU count)
            size_t held = 0;
            S.cap = 0;
            S.state_nctu = -1;
            if (!seq_grow(&S.d_state, &held, state_bytes(seqs[j].geom.nctu))) {
                drop_states(s);
                return ldp_set_err(s, ETHCNN_ERR_NOMEM, "%s: %zu bytes of state do not fit (%s %d)", who, state_bytes(seqs[j].geom.nctu), item, j);
            }
            S.cap = (seqs[j].geom.nctu + 15) / 16 * 16;
        }
    }
    // the front-end's workspace at the size of the largest pass of the call: it does not grow (and wait for the stream) between
    // sequences.  Behind the memory check, so a failure here is one "after that point": the resident states are dropped
    if (int rc = ensure_workspace(c, (int)front_ctus, 1)) {
        drop_states(s);
        return ldp_set_err(s, rc, "%s (the resident states of the %s were dropped)", c->err.c_str(), form);
    }
    // ---- the chunk loop.  A resident state is advanced in place: a block stores only its own columns (ethcnn_lstm_seq.h)
    c->done_armed = 0;
    for (int j = 0; j < nseqs; ++j) s->s[j].state_nctu = -1;  // until every frame has been enqueued
    for (int64_t f0 = 0; f0 < longest; f0 += Fc) {
        SeqBatchRow rows[kLstmSeqBatchMax];
        float thr1[kLstmSeqBatchMax], thr2[kLstmSeqBatchMax];  // by row: the pair follows the sequence index, not the row position
        int k = 0;
        for (int j = 0; j < nseqs; ++j) {
            const LdpSeq& q = seqs[j];
            if (f0 >= q.nframes) continue;  // this sequence has ended
            ldp_set_gates_of(s, j, &thr1[k], &thr2[k]);
            const int n = q.geom.nctu, f = (int)std::min<int64_t>(Fc, q.nframes - f0);
            float* const vec = s->d_vec + slice[j];
            if (int rc = seq_front(c, q.d_luma + f0 * q.geom.frame_stride, q.geom, f, vec)) {
                drop_states(s);
                return ldp_set_err(s, rc, "%s %d: %s (the resident states of the %s were dropped)", item, j, c->err.c_str(), form);
            }
            float* const state = s->s[j].d_state;
            rows[k++] = {vec, (f0 || !q.d_state_in) ? state : q.d_state_in, state, q.d_lstm, q.d_probs + (size_t)f0 * n * kNOut,
                         lstm_seq_efs0(q.qp), n, f, q.i_frame_first + (int)f0};
        }
        const hipError_t e = seq_launch(c, rows, k, thr1, thr2);
        if (e != hipSuccess) {
            drop_states(s);
            return ldp_set_err(s, ETHCNN_ERR_DEVICE, "launch failed: %s (the resident states of the %s were dropped)", hipGetErrorString(e), form);
        }
    }
    for (int j = 0; j < nseqs; ++j) s->s[j].state_nctu = seqs[j].geom.nctu;
    const int rc = serial_end(c);
    return rc ? ldp_set_err(s, rc, "%s", c->err.c_str()) : ETHCNN_OK;
}
