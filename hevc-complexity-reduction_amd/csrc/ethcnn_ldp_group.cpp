// ethcnn_ldp_group.cpp -- config #5 offline, group form (include/ethcnn.h): K residual sequences of one geometry, each with its own
// ETH-LSTM bundle, QP, state and output, through ONE recurrence launch per run of frames.  Member m's result is what
// ethcnn_ldp_sequence_device gives on a context that holds m's bundle, bit for bit.  A group is a set (ethcnn_ldp_set.h) whose
// sequence m uses bundle m: this file holds the entries, the byte formula and the checks of the device entry.
#include "ethcnn_ldp_set.h"

extern "C" int64_t ethcnn_ldp_group_bytes(int w, int h, int nframes, int chunk_frames, int k) {
    if (w <= 0 || h <= 0 || nframes <= 0 || chunk_frames < 0 || k < 1 || k > kLstmSeqGroupMax) return ETHCNN_ERR_ARG;
    const int64_t nctu = (int64_t)((w + 63) / 64) * ((h + 63) / 64), cap = (nctu + 15) / 16 * 16;
    const int64_t F = std::min<int64_t>(nframes, seq_chunk_frames(k * nctu, chunk_frames));
    return k * F * nctu * kNVec * 4 + k * cap * kLdpStateFloats * 4;
}

extern "C" int ethcnn_ldp_group_create(ethcnn_ctx* c, int k, ethcnn_ldp_group** out) {
    return ldp_set_create(c, k, k, "ethcnn_ldp_group_create", "members", out);
}
extern "C" void ethcnn_ldp_group_destroy(ethcnn_ldp_group* g) { ldp_set_release(g); delete g; }
extern "C" const char* ethcnn_ldp_group_last_error(const ethcnn_ldp_group* g) { return g ? g->err.c_str() : "LDP group is NULL"; }
extern "C" int ethcnn_ldp_group_count(const ethcnn_ldp_group* g) { return g ? g->nb : ETHCNN_ERR_ARG; }
extern "C" int ethcnn_ldp_group_load_lstm_blob(ethcnn_ldp_group* g, int m, const float* blob, size_t nfloats) {
    return ldp_set_load_blob(g, m, blob, nfloats, "ethcnn_ldp_group_load_lstm_blob", "member");
}
extern "C" int ethcnn_ldp_group_load_lstm_synthetic(ethcnn_ldp_group* g, int m, uint64_t seed, double head_gain) {
    return ldp_set_load_synthetic(g, m, seed, head_gain, "ethcnn_ldp_group_load_lstm_synthetic", "member");
}
extern "C" int ethcnn_ldp_group_load_lstm_checkpoint(ethcnn_ldp_group* g, int m, const char* prefix) {
    return ldp_set_load_checkpoint(g, m, prefix, "ethcnn_ldp_group_load_lstm_checkpoint", "member");
}
extern "C" int ethcnn_ldp_group_get_lstm_blob(ethcnn_ldp_group* g, int m, float* out, size_t nfloats) {
    return ldp_set_get_blob(g, m, out, nfloats, "ethcnn_ldp_group_get_lstm_blob", "member");
}
extern "C" int ethcnn_ldp_group_set_chunk(ethcnn_ldp_group* g, int frames) { return ldp_set_chunk(g, frames, "ethcnn_ldp_group_set_chunk"); }
extern "C" int64_t ethcnn_ldp_group_state_ctus(ethcnn_ldp_group* g, int m) { return ldp_set_state_ctus(g, m, "ethcnn_ldp_group_state_ctus", "member"); }
extern "C" int ethcnn_ldp_group_get_state(ethcnn_ldp_group* g, int m, float* out, size_t nfloats) {
    return ldp_set_get_state(g, m, out, nfloats, "ethcnn_ldp_group_get_state", "member");
}
extern "C" int ethcnn_ldp_set_thresholds_group(ethcnn_ldp_group* g, int m, float thr_l1_lower, float thr_l2_lower) {
    return ldp_set_set_gates(g, m, thr_l1_lower, thr_l2_lower, "ethcnn_ldp_set_thresholds_group", "member");
}
extern "C" int ethcnn_ldp_clear_thresholds_group(ethcnn_ldp_group* g, int m) { return ldp_set_clear_gates(g, m, "ethcnn_ldp_clear_thresholds_group", "member"); }
extern "C" int ethcnn_ldp_get_thresholds_group(ethcnn_ldp_group* g, int m, float* thr_l1_lower, float* thr_l2_lower, int* own) {
    return ldp_set_get_gates(g, m, thr_l1_lower, thr_l2_lower, own, "ethcnn_ldp_get_thresholds_group", "member");
}

extern "C" int ethcnn_ldp_group_sequence_device(ethcnn_ldp_group* g, const uint8_t* const* d_luma, int w, int h, ptrdiff_t pitch, ptrdiff_t fstride,
                                                int nframes, const int* qp, int i_first, const float* const* d_state_in, float* const* d_probs) {
    if (!g) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = g->c;
    const int K = g->nb;
    // ---- checks: nothing is allocated or enqueued before they pass
    if (c->ldp.open || c->ai.open) return ldp_set_err(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_sequence: a streamed call has not been ended");
    if (!c->have_weights) return ldp_set_err(g, ETHCNN_ERR_NOWEIGHTS, "no CNN weights loaded");
    for (int m = 0; m < K; ++m)
        if (!g->b[m].have) return ldp_set_err(g, ETHCNN_ERR_NOWEIGHTS, "member %d has no ETH-LSTM bundle loaded (ethcnn_ldp_group_load_lstm_*)", m);
    if (!d_luma || !qp || !d_probs) return ldp_set_err(g, ETHCNN_ERR_ARG, "null pointer");
    for (int m = 0; m < K; ++m)
        if (!d_luma[m] || !d_probs[m]) return ldp_set_err(g, ETHCNN_ERR_ARG, "null pointer (member %d)", m);
    for (int m = 0; m < K; ++m) {  // lstm_seq_level reads a state as float4; d_probs is touched dword by dword
        if (d_state_in && (uintptr_t)d_state_in[m] % 16) return ldp_set_err(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_sequence: d_state_in[%d] is not 16-byte aligned", m);
        if ((uintptr_t)d_probs[m] % 4) return ldp_set_err(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_sequence: d_probs[%d] is not 4-byte aligned", m);
    }
    if (w <= 0 || h <= 0 || pitch < w) return ldp_set_err(g, ETHCNN_ERR_ARG, "bad geometry");
    if (nframes <= 0) return ldp_set_err(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_sequence: nframes must be positive");
    if (i_first < 0) return ldp_set_err(g, ETHCNN_ERR_ARG, "ethcnn_ldp_group_sequence: i_frame_first must not be negative");
    const int nctu = ((w + 63) / 64) * ((h + 63) / 64);
    if (i_first > 1)
        for (int m = 0; m < K; ++m)
            if (!(d_state_in && d_state_in[m]) && g->s[m].state_nctu != nctu)
                return ldp_set_err(g, ETHCNN_ERR_ARG, "ethcnn_ldp_step: frame %d needs the previous frame's state, but none is resident for %d CTUs (member %d)",
                                   i_first, nctu, m);
    FrameGeom geom;
    if (int rc = make_geom(c, w, h, pitch, fstride, &geom)) return ldp_set_err(g, rc, "%s", c->err.c_str());
    LdpSeq seqs[kLstmSeqGroupMax];
    for (int m = 0; m < K; ++m) seqs[m] = {d_luma[m], geom, nframes, i_first, qp[m], g->b[m].d_lstm, d_state_in ? d_state_in[m] : nullptr, d_probs[m]};
    return ldp_set_run(g, seqs, K, "ethcnn_ldp_group_sequence", "member", "group");
}
