// ethcnn_ldp_batch.cpp -- config #5 offline, batch form (include/ethcnn.h): up to 32 residual sequences of different geometry, length
// and first frame number through ONE recurrence launch and ONE gate launch per chunk.  Sequence j's result is what
// ethcnn_ldp_sequence_device gives on a context that holds bundle seqs[j].bundle, bit for bit.  A batch is a set (ethcnn_ldp_set.h)
// whose sequences name their bundles: this file holds the entries, the byte formula, the plan and the checks of the device entry.
#include "ethcnn_ldp_set.h"

namespace {
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
    const int64_t Fc = seq_chunk_frames(sum, chunk_frames);
    int64_t bytes = 0;
    for (int j = 0; j < nseqs; ++j) {
        const int64_t nctu = (int64_t)((widths[j] + 63) / 64) * ((heights[j] + 63) / 64);
        bytes += std::min<int64_t>(nframes[j], Fc) * nctu * kNVec * 4 + (nctu + 15) / 16 * 16 * kLdpStateFloats * 4;
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
    const int64_t Fc = std::min<int64_t>(seq_chunk_frames(sum, chunk_frames), INT32_MAX), nchunks = (longest + Fc - 1) / Fc;
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
    return ldp_set_create(c, nbundles, kLstmSeqBatchMax, "ethcnn_ldp_batch_create", "bundles", out);
}
extern "C" void ethcnn_ldp_batch_destroy(ethcnn_ldp_batch* b) { ldp_set_release(b); delete b; }
extern "C" const char* ethcnn_ldp_batch_last_error(const ethcnn_ldp_batch* b) { return b ? b->err.c_str() : "LDP batch is NULL"; }
extern "C" int ethcnn_ldp_batch_bundles(const ethcnn_ldp_batch* b) { return b ? b->nb : ETHCNN_ERR_ARG; }
extern "C" int ethcnn_ldp_batch_load_lstm_blob(ethcnn_ldp_batch* b, int i, const float* blob, size_t nfloats) {
    return ldp_set_load_blob(b, i, blob, nfloats, "ethcnn_ldp_batch_load_lstm_blob", "bundle");
}
extern "C" int ethcnn_ldp_batch_load_lstm_synthetic(ethcnn_ldp_batch* b, int i, uint64_t seed, double head_gain) {
    return ldp_set_load_synthetic(b, i, seed, head_gain, "ethcnn_ldp_batch_load_lstm_synthetic", "bundle");
}
extern "C" int ethcnn_ldp_batch_load_lstm_checkpoint(ethcnn_ldp_batch* b, int i, const char* prefix) {
    return ldp_set_load_checkpoint(b, i, prefix, "ethcnn_ldp_batch_load_lstm_checkpoint", "bundle");
}
extern "C" int ethcnn_ldp_batch_get_lstm_blob(ethcnn_ldp_batch* b, int i, float* out, size_t nfloats) {
    return ldp_set_get_blob(b, i, out, nfloats, "ethcnn_ldp_batch_get_lstm_blob", "bundle");
}
extern "C" int ethcnn_ldp_batch_set_chunk(ethcnn_ldp_batch* b, int frames) { return ldp_set_chunk(b, frames, "ethcnn_ldp_batch_set_chunk"); }
extern "C" int64_t ethcnn_ldp_batch_state_ctus(ethcnn_ldp_batch* b, int j) { return ldp_set_state_ctus(b, j, "ethcnn_ldp_batch_state_ctus", "sequence index"); }
extern "C" int ethcnn_ldp_batch_get_state(ethcnn_ldp_batch* b, int j, float* out, size_t nfloats) {
    return ldp_set_get_state(b, j, out, nfloats, "ethcnn_ldp_batch_get_state", "sequence index");
}
extern "C" int ethcnn_ldp_set_thresholds_batch(ethcnn_ldp_batch* b, int j, float thr_l1_lower, float thr_l2_lower) {
    return ldp_set_set_gates(b, j, thr_l1_lower, thr_l2_lower, "ethcnn_ldp_set_thresholds_batch", "sequence index");
}
extern "C" int ethcnn_ldp_clear_thresholds_batch(ethcnn_ldp_batch* b, int j) {
    return ldp_set_clear_gates(b, j, "ethcnn_ldp_clear_thresholds_batch", "sequence index");
}
extern "C" int ethcnn_ldp_get_thresholds_batch(ethcnn_ldp_batch* b, int j, float* thr_l1_lower, float* thr_l2_lower, int* own) {
    return ldp_set_get_gates(b, j, thr_l1_lower, thr_l2_lower, own, "ethcnn_ldp_get_thresholds_batch", "sequence index");
}

extern "C" int ethcnn_ldp_batch_run_device(ethcnn_ldp_batch* b, const ethcnn_ldp_batch_seq* seqs, int nseqs) {
    if (!b) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = b->c;
    // ---- checks: nothing is allocated or enqueued before they pass
    if (c->ldp.open || c->ai.open) return ldp_set_err(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: a streamed call has not been ended");
    if (!c->have_weights) return ldp_set_err(b, ETHCNN_ERR_NOWEIGHTS, "no CNN weights loaded");
    if (nseqs < 1 || nseqs > kLstmSeqBatchMax) return ldp_set_err(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: %d sequences (1..%d)", nseqs, kLstmSeqBatchMax);
    if (!seqs) return ldp_set_err(b, ETHCNN_ERR_ARG, "null pointer");
    LdpSeq run[kLstmSeqBatchMax];
    for (int j = 0; j < nseqs; ++j) {
        const ethcnn_ldp_batch_seq& q = seqs[j];
        if (q.bundle < 0 || q.bundle >= b->nb || !b->b[q.bundle].have)
            return ldp_set_err(b, ETHCNN_ERR_NOWEIGHTS, "sequence %d: bundle %d is %s (ethcnn_ldp_batch_load_lstm_*)", j, q.bundle,
                               q.bundle < 0 || q.bundle >= b->nb ? "outside the batch's bundles" : "empty");
        if (!q.d_luma || !q.d_probs) return ldp_set_err(b, ETHCNN_ERR_ARG, "null pointer (sequence %d)", j);
        // lstm_seq_level reads a state as float4; d_probs is touched dword by dword
        if ((uintptr_t)q.d_state_in % 16) return ldp_set_err(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: d_state_in of sequence %d is not 16-byte aligned", j);
        if ((uintptr_t)q.d_probs % 4) return ldp_set_err(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: d_probs of sequence %d is not 4-byte aligned", j);
        if (q.width <= 0 || q.height <= 0 || q.pitch < q.width) return ldp_set_err(b, ETHCNN_ERR_ARG, "bad geometry (sequence %d)", j);
        if (q.nframes <= 0) return ldp_set_err(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: nframes must be positive (sequence %d)", j);
        if (q.i_frame_first < 1)
            return ldp_set_err(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: i_frame_first %d of sequence %d: frame 0 is the intra picture, a batch starts at frame 1 or later",
                               q.i_frame_first, j);
        FrameGeom geom;
        if (int rc = make_geom(c, q.width, q.height, q.pitch, q.frame_stride, &geom)) return ldp_set_err(b, rc, "sequence %d: %s", j, c->err.c_str());
        if (q.i_frame_first > 1 && !q.d_state_in && b->s[j].state_nctu != geom.nctu)
            return ldp_set_err(b, ETHCNN_ERR_ARG, "ethcnn_ldp_step: frame %d needs the previous frame's state, but none is resident for %d CTUs (sequence %d)",
                               q.i_frame_first, geom.nctu, j);
        run[j] = {q.d_luma, geom, q.nframes, q.i_frame_first, q.qp, b->b[q.bundle].d_lstm, q.d_state_in, q.d_probs};
    }
    for (int j = 0; j < nseqs; ++j) {
        const size_t pj = (size_t)run[j].nframes * run[j].geom.nctu * kNOut * 4;
        for (int i = 0; i < nseqs; ++i) {
            if (i == j) continue;
            if (overlap(run[j].d_probs, pj, run[i].d_probs, (size_t)run[i].nframes * run[i].geom.nctu * kNOut * 4) ||
                (run[i].d_state_in && run[i].i_frame_first > 1 && overlap(run[j].d_probs, pj, run[i].d_state_in, (size_t)run[i].geom.nctu * kLdpStateFloats * 4)))
                return ldp_set_err(b, ETHCNN_ERR_ARG, "ethcnn_ldp_batch_run: d_probs of sequence %d overlaps a buffer of sequence %d", j, i);
        }
    }
    return ldp_set_run(b, run, nseqs, "ethcnn_ldp_batch_run", "sequence", "batch");
}
