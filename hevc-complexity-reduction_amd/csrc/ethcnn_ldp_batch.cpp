// ethcnn_ldp_batch.cpp -- config #5 offline, batch form (include/ethcnn.h): up to 32 residual sequences of different geometry, length
// and first frame number through ONE recurrence launch and ONE gate launch per chunk.  Sequence j's result is what
// ethcnn_ldp_sequence_device gives on a context that holds bundle seqs[j].bundle, bit for bit: the same front-end (seq_front, per
// sequence) and the same kernel bodies (ethcnn_lstm_seq.hip), which take n, F and i_frame0 from the sequence's own row.
#include "ethcnn_ctx.h"
#include "ethcnn_ldp_batch.h"

namespace {
int berr(ethcnn_ldp_batch* b, int code, const char* fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    b->err = buf;
    return code;
}
#define BCHK(b, call)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return berr((b), ETHCNN_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

constexpr int64_t kStateFloats = 2 * kNVec;  // (c, h) of a CTU
constexpr int64_t kVecBytes = kNVec * 4;     // the front-end's vector of a CTU

// frames per chunk, common to all sequences of a call: the caller's figure, else what keeps a chunk's vectors within 256 MB
int64_t batch_fc(int64_t sum_nctu, int chunk) {
    return chunk > 0 ? (int64_t)chunk : std::max<int64_t>(1, (int64_t)(256 << 20) / (sum_nctu * kVecBytes));
}

int check_bundle(ethcnn_ldp_batch* b, int i, const char* who) {
    if (i < 0 || i >= b->nb) return berr(b, ETHCNN_ERR_ARG, "%s: bundle %d outside 0..%d", who, i, b->nb - 1);
    return 0;
}
int check_seq(ethcnn_ldp_batch* b, int j, const char* who) {
    if (j < 0 || j >= kLstmSeqBatchMax) return berr(b, ETHCNN_ERR_ARG, "%s: sequence index %d outside 0..%d", who, j, kLstmSeqBatchMax - 1);
    return 0;
}

int upload_bundle(ethcnn_ldp_batch* b, int i) {
    ethcnn_ldp_batch::Bundle& B = b->b[i];
    const int rc = upload_lstm_image(b->c, B.blob.data(), &B.d_lstm);
    if (rc) {
        B.have = false;  // (the image may be half written)
        return berr(b, rc, "bundle %d: %s", i, b->c->err.c_str());
    }
    B.have = true;
    return ETHCNN_OK;
}

void drop_states(ethcnn_ldp_batch* b) {
    for (auto& s : b->s) s.state_nctu = -1;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}
}  // namespace

extern "C" int64_t ethcnn_ldp_batch_bytes(const int* widths, const int* heights, const int* nframes, int nseqs, int chunk_frames) {
    if (!widths || !heights || !nframes || nseqs < 1 || nseqs > kLstmSeqBatchMax || chunk_frames < 0) return ETHCNN_ERR_ARG;
    int64_t sum = 0;
    for (int j = 0; j < nseqs; ++j) {
        if (widths[j] <= 0 || heights[j] <= 0 || nframes[j] <= 0) return ETHCNN_ERR_ARG;
        sum += (int64_t)((widths[j] + 63) / 64) * ((heights[j] + 63) / 64);
    }
    const int64_t Fc = batch_fc(sum, chunk_frames);
    int64_t bytes = 0;
    for (int j = 0; j < nseqs; ++j) {
        const int64_t nctu = (int64_t)((widths[j] + 63) / 64) * ((heights[j] + 63) / 64);
        bytes += std::min<int64_t>(nframes[j], Fc) * nctu * kVecBytes + (nctu + 15) / 16 * 16 * kStateFloats * 4;
    }
    return bytes;
}

extern "C" int ethcnn_ldp_batch_plan(const int* nctus, const int* nframes, int nseqs, int chunk_frames, int* fc_out, int* nchunks_out, int* chunks_out,
                                     int max_chunks) {
    if (!nctus || !nframes || nseqs < 1 || nseqs > kLstmSeqBatchMax || chunk_frames < 0 || max_chunks < 0 || (max_chunks && !chunks_out)) return ETHCNN_ERR_ARG;
    int64_t sum = 0, longest = 0;
    for (int j = 0; j < nseqs; ++j) {
        if (nctus[j] <= 0 || nframes[j] <= 0) return ETHCNN_ERR_ARG;
        sum += nctus[j];
        longest = std::max<int64_t>(longest, nframes[j]);
    }
    const int64_t Fc = std::min<int64_t>(batch_fc(sum, chunk_frames), INT32_MAX), nchunks = (longest + Fc - 1) / Fc;
    if (fc_out) *fc_out = (int)Fc;
    if (nchunks_out) *nchunks_out = (int)nchunks;
    for (int64_t t = 0; t < nchunks && t < max_chunks; ++t) {
        int64_t row[4] = {0, 0, 0, 0};
        for (int j = 0; j < nseqs; ++j)
            if (t * Fc < nframes[j]) {
                int64_t blocks[3];
                lstm_seq_blocks(nctus[j], blocks);
                ++row[0];
                for (int lv = 0; lv < 3; ++lv) row[1 + lv] += blocks[lv];
            }
        for (int i = 0; i < 4; ++i) chunks_out[4 * t + i] = (int)row[i];
    }
    return ETHCNN_OK;
}

extern "C" int ethcnn_ldp_batch_create(ethcnn_ctx* c, int nbundles, ethcnn_ldp_batch** out) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "null output pointer");
    *out = nullptr;
    if (nbundles < 1 || nbundles > kLdpBatchBundles) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_create: %d bundles (1..%d)", nbundles, kLdpBatchBundles);
    ethcnn_ldp_batch* b = new (std::nothrow) ethcnn_ldp_batch;
    if (!b) return set_err(c, ETHCNN_ERR_NOMEM, "out of memory");
    b->c = c;
    b->nb = nbundles;
    *out = b;
    return ETHCNN_OK;
}

extern "C" void ethcnn_ldp_batch_destroy(ethcnn_ldp_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->c->device);
    (void)hipStreamSynchronize(b->c->stream);
    for (auto& B : b->b)
        if (B.d_lstm) (void)hipFree(B.d_lstm);
    for (auto& s : b->s)
        if (s.d_state) (void)hipFree(s.d_state);
    if (b->d_vec) (void)hipFree(b->d_vec);
    delete b;
}

extern "C" const char* ethcnn_ldp_batch_last_error(const ethcnn_ldp_batch* b) { return b ? b->err.c_str() : "LDP batch is NULL"; }
extern "C" int ethcnn_ldp_batch_bundles(const ethcnn_ldp_batch* b) { return b ? b->nb : ETHCNN_ERR_ARG; }

extern "C" int ethcnn_ldp_batch_load_lstm_blob(ethcnn_ldp_batch* b, int i, const float* blob, size_t nfloats) {
    if (!b) return ETHCNN_ERR_ARG;
    if (int rc = check_bundle(b, i, "ethcnn_ldp_batch_load_lstm_blob")) return rc;
    if (!blob) return berr(b, ETHCNN_ERR_ARG, "null pointer");
    if (nfloats != kLstmBlobFloats) return berr(b, ETHCNN_ERR_ARG, "LSTM blob must hold %zu floats, got %zu", (size_t)kLstmBlobFloats, nfloats);
    b->b[i].blob.assign(blob, blob + nfloats);
    return upload_bundle(b, i);
}

extern "C" int ethcnn_ldp_batch_load_lstm_synthetic(ethcnn_ldp_batch* b, int i, uint64_t seed, double head_gain) {
    if (!b) return ETHCNN_ERR_ARG;
    if (int rc = check_bundle(b, i, "ethcnn_ldp_batch_load_lstm_synthetic")) return rc;
    b->b[i].blob.resize(kLstmBlobFloats);
    synth_lstm_blob(seed, head_gain, b->b[i].blob.data());
    return upload_bundle(b, i);
}

extern "C" int ethcnn_ldp_batch_load_lstm_checkpoint(ethcnn_ldp_batch* b, int i, const char* prefix) {
    if (!b) return ETHCNN_ERR_ARG;
    if (int rc = check_bundle(b, i, "ethcnn_ldp_batch_load_lstm_checkpoint")) return rc;
    if (!prefix) return berr(b, ETHCNN_ERR_ARG, "null pointer");
    std::vector<float> blob(kLstmBlobFloats);
    char err[400];
    const int rc = ckpt_load_table(prefix, kLstmTensors, kNumLstmTensors, blob.data(), err, sizeof err);
    if (rc) return berr(b, rc, "bundle %d: %s", i, err);  // (the bundle keeps what it had)
    b->b[i].blob.swap(blob);
    return upload_bundle(b, i);
}

extern "C" int ethcnn_ldp_batch_get_lstm_blob(ethcnn_ldp_batch* b, int i, float* out, size_t nfloats) {
    if (!b) return ETHCNN_ERR_ARG;
    if (int rc = check_bundle(b, i, "ethcnn_ldp_batch_get_lstm_blob")) return rc;
    if (!out || nfloats != kLstmBlobFloats) return berr(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_get_lstm_blob: a buffer of %zu floats", (size_t)kLstmBlobFloats);
    if (!b->b[i].have) return berr(b, ETHCNN_ERR_NOWEIGHTS, "bundle %d holds no ETH-LSTM bundle", i);
    std::memcpy(out, b->b[i].blob.data(), nfloats * 4);
    return ETHCNN_OK;
}

extern "C" int ethcnn_ldp_batch_set_chunk(ethcnn_ldp_batch* b, int frames) {
    if (!b) return ETHCNN_ERR_ARG;
    if (frames < 0) return berr(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_set_chunk: %d frames", frames);
    b->chunk = frames;
    return ETHCNN_OK;
}

extern "C" int64_t ethcnn_ldp_batch_state_ctus(ethcnn_ldp_batch* b, int j) {
    if (!b) return ETHCNN_ERR_ARG;
    if (int rc = check_seq(b, j, "ethcnn_ldp_batch_state_ctus")) return rc;
    return b->s[j].state_nctu < 0 ? 0 : b->s[j].state_nctu;
}

extern "C" int ethcnn_ldp_batch_get_state(ethcnn_ldp_batch* b, int j, float* out, size_t nfloats) {
    if (!b) return ETHCNN_ERR_ARG;
    if (int rc = check_seq(b, j, "ethcnn_ldp_batch_get_state")) return rc;
    if (!out) return berr(b, ETHCNN_ERR_ARG, "null pointer");
    const ethcnn_ldp_batch::Seq& S = b->s[j];
    if (S.state_nctu < 0) return berr(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_get_state: sequence index %d has no resident state", j);
    if (nfloats != (size_t)S.state_nctu * kStateFloats)
        return berr(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_get_state: the resident state of sequence index %d holds %zu floats, not %zu", j,
                    (size_t)S.state_nctu * kStateFloats, nfloats);
    ethcnn_ctx* c = b->c;
    BCHK(b, hipSetDevice(c->device));
    BCHK(b, hipMemcpyAsync(out, S.d_state, nfloats * 4, hipMemcpyDeviceToHost, c->stream));
    BCHK(b, hipStreamSynchronize(c->stream));
    return ETHCNN_OK;
}

extern "C" int ethcnn_ldp_batch_run_device(ethcnn_ldp_batch* b, const ethcnn_ldp_batch_seq* seqs, int nseqs) {
    if (!b) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = b->c;
    // ---- checks: nothing is allocated or enqueued before they pass
    if (c->ldp.open || c->ai.open) return berr(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: a streamed call has not been ended");
    if (!c->have_weights) return berr(b, ETHCNN_ERR_NOWEIGHTS, "no CNN weights loaded");
    if (nseqs < 1 || nseqs > kLstmSeqBatchMax) return berr(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: %d sequences (1..%d)", nseqs, kLstmSeqBatchMax);
    if (!seqs) return berr(b, ETHCNN_ERR_ARG, "null pointer");
    FrameGeom geom[kLstmSeqBatchMax];
    int64_t sum_nctu = 0, longest = 0;
    for (int j = 0; j < nseqs; ++j) {
        const ethcnn_ldp_batch_seq& q = seqs[j];
        if (q.bundle < 0 || q.bundle >= b->nb || !b->b[q.bundle].have)
            return berr(b, ETHCNN_ERR_NOWEIGHTS, "sequence %d: bundle %d is %s (ethcnn_ldp_batch_load_lstm_*)", j, q.bundle,
                        q.bundle < 0 || q.bundle >= b->nb ? "outside the batch's bundles" : "empty");
        if (!q.d_luma || !q.d_probs) return berr(b, ETHCNN_ERR_ARG, "null pointer (sequence %d)", j);
        // lstm_seq_level reads a state as float4; d_probs is touched dword by dword
        if ((uintptr_t)q.d_state_in % 16) return berr(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: d_state_in of sequence %d is not 16-byte aligned", j);
        if ((uintptr_t)q.d_probs % 4) return berr(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: d_probs of sequence %d is not 4-byte aligned", j);
        if (q.width <= 0 || q.height <= 0 || q.pitch < q.width) return berr(b, ETHCNN_ERR_ARG, "bad geometry (sequence %d)", j);
        if (q.nframes <= 0) return berr(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: nframes must be positive (sequence %d)", j);
        if (q.i_frame_first < 1)
            return berr(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: i_frame_first %d of sequence %d: frame 0 is the intra picture, a batch starts at frame 1 or later",
                        q.i_frame_first, j);
        if (int rc = make_geom(c, q.width, q.height, q.pitch, q.frame_stride, &geom[j])) return berr(b, rc, "sequence %d: %s", j, c->err.c_str());
        if (q.i_frame_first > 1 && !q.d_state_in && b->s[j].state_nctu != geom[j].nctu)
            return berr(b, ETHCNN_ERR_ARG, "ethcnn_ldp_step: frame %d needs the previous frame's state, but none is resident for %d CTUs (sequence %d)",
                        q.i_frame_first, geom[j].nctu, j);
        sum_nctu += geom[j].nctu;
        longest = std::max<int64_t>(longest, q.nframes);
    }
    for (int j = 0; j < nseqs; ++j) {
        const size_t pj = (size_t)seqs[j].nframes * geom[j].nctu * kNOut * 4;
        for (int i = 0; i < nseqs; ++i) {
            if (i == j) continue;
            if (overlap(seqs[j].d_probs, pj, seqs[i].d_probs, (size_t)seqs[i].nframes * geom[i].nctu * kNOut * 4) ||
                (seqs[i].d_state_in && seqs[i].i_frame_first > 1 && overlap(seqs[j].d_probs, pj, seqs[i].d_state_in, (size_t)geom[i].nctu * kStateFloats * 4)))
                return berr(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: d_probs of sequence %d overlaps a buffer of sequence %d", j, i);
        }
    }
    // ---- buffers: refused with the whole sum before anything is allocated
    const int64_t Fc = batch_fc(sum_nctu, b->chunk);
    size_t slice[kLstmSeqBatchMax + 1];  // sequence j's vectors start at float slice[j]
    slice[0] = 0;
    int64_t total = 0, front_ctus = 0;
    for (int j = 0; j < nseqs; ++j) {
        const int64_t nf = std::min<int64_t>(seqs[j].nframes, Fc);
        slice[j + 1] = slice[j] + (size_t)nf * geom[j].nctu * kNVec;
        total += nf * geom[j].nctu * kVecBytes + (int64_t)((geom[j].nctu + 15) / 16 * 16) * kStateFloats * 4;
        front_ctus = std::max<int64_t>(front_ctus, std::min<int64_t>((int64_t)geom[j].nctu * nf, c->max_ctus));
    }
    const size_t vb = slice[nseqs] * 4;
    BCHK(b, hipSetDevice(c->device));
    size_t grow = 0, back = 0;
    if (vb > b->vec_cap) grow += vb, back += b->vec_cap;
    for (int j = 0; j < nseqs; ++j)
        if (geom[j].nctu > b->s[j].cap) grow += (size_t)((geom[j].nctu + 15) / 16 * 16) * kStateFloats * 4, back += (size_t)b->s[j].cap * kStateFloats * 4;
    if (grow) {
        size_t free_b = 0, total_b = 0;
        BCHK(b, hipMemGetInfo(&free_b, &total_b));
        if (grow > free_b + back)
            return berr(b, ETHCNN_ERR_NOMEM, "ethcnn_ldp_batch_run: %d sequences in chunks of %lld frames hold %lld bytes on the device (ethcnn_ldp_batch_bytes); %zu are free",
                        nseqs, (long long)Fc, (long long)total, free_b + back);
        BCHK(b, hipStreamSynchronize(c->stream));
        if (!seq_grow(&b->d_vec, &b->vec_cap, vb)) return berr(b, ETHCNN_ERR_NOMEM, "ethcnn_ldp_batch_run: %zu bytes of vectors do not fit", vb);
        for (int j = 0; j < nseqs; ++j) {
            ethcnn_ldp_batch::Seq& S = b->s[j];
            if (geom[j].nctu <= S.cap) continue;
            // (this index does not continue from its resident state: that belongs to a smaller CTU count)
            const int cap = (geom[j].nctu + 15) / 16 * 16;
            size_t held = 0;
            S.cap = 0;
            S.state_nctu = -1;
            if (!seq_grow(&S.d_state, &held, (size_t)cap * kStateFloats * 4)) {
                drop_states(b);
                return berr(b, ETHCNN_ERR_NOMEM, "ethcnn_ldp_batch_run: %zu bytes of state do not fit (sequence %d)", (size_t)cap * kStateFloats * 4, j);
            }
            S.cap = cap;
        }
    }
    // the front-end's workspace at the size of the largest pass of the call: it does not grow (and wait for the stream) between
    // sequences.  Behind the memory check, so a failure here is one "after that point": the resident states are dropped
    if (int rc = ensure_workspace(c, (int)front_ctus, 1)) {
        drop_states(b);
        return berr(b, rc, "%s (the resident states of the batch were dropped)", c->err.c_str());
    }
    // ---- the chunk loop.  A resident state is advanced in place: a block stores only its own columns (ethcnn_lstm_seq.h)
    c->done_armed = 0;
    const float* sin[kLstmSeqBatchMax];
    for (int j = 0; j < nseqs; ++j) {
        sin[j] = seqs[j].i_frame_first > 1 ? (seqs[j].d_state_in ? seqs[j].d_state_in : b->s[j].d_state) : nullptr;
        b->s[j].state_nctu = -1;  // until every frame has been enqueued
    }
    for (int64_t f0 = 0; f0 < longest; f0 += Fc) {
        SeqBatchRow rows[kLstmSeqBatchMax];
        float* probs[kLstmSeqBatchMax];
        int n[kLstmSeqBatchMax], nf[kLstmSeqBatchMax], k = 0;
        long ctu_frames = 0;
        for (int j = 0; j < nseqs; ++j) {
            const ethcnn_ldp_batch_seq& q = seqs[j];
            if (f0 >= q.nframes) continue;  // this sequence has ended
            const int f = (int)std::min<int64_t>(Fc, q.nframes - f0);
            float* const vec = b->d_vec + slice[j];
            if (int rc = seq_front(c, q.d_luma + f0 * q.frame_stride, geom[j], f, vec)) {
                drop_states(b);
                return berr(b, rc, "sequence %d: %s (the resident states of the batch were dropped)", j, c->err.c_str());
            }
            probs[k] = q.d_probs + (size_t)f0 * geom[j].nctu * kNOut;
            n[k] = geom[j].nctu, nf[k] = f;
            rows[k] = {{vec, sin[j], b->s[j].d_state, b->b[q.bundle].d_lstm, probs[k], lstm_seq_efs0(q.qp)}, geom[j].nctu, f, q.i_frame_first + (int)f0};
            sin[j] = b->s[j].d_state;
            ctu_frames += (long)geom[j].nctu * f;
            ++k;
        }
        { StageTimer t(c, ETHCNN_STAGE_HEADS, ctu_frames); launch_lstm_seq_batch(rows, k, c->stream); }
        { StageTimer t(c, ETHCNN_STAGE_GATE); launch_lstm_seq_gates_batch(probs, n, nf, k, c->thr1, c->thr2, c->stream); }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            drop_states(b);
            return berr(b, ETHCNN_ERR_DEVICE, "launch failed: %s (the resident states of the batch were dropped)", hipGetErrorString(e));
        }
    }
    for (int j = 0; j < nseqs; ++j) b->s[j].state_nctu = geom[j].nctu;
    const int rc = serial_end(c);
    return rc ? berr(b, rc, "%s", c->err.c_str()) : ETHCNN_OK;
}
