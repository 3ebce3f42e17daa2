// ethcnn_ldp.cpp -- config #5: resi_cnn vectors, one ETH-LSTM step, the per-frame Low-Delay-P calls (resident state, streamed input),
// and the offline calls over a whole residual sequence (at the end of the file)
#include "ethcnn_ctx.h"
#include "ethcnn_lstm_seq.h"

// -------------------------------------------------------------- config #5 -----------
extern "C" int ethcnn_resi_vectors_device(ethcnn_ctx* c, const uint8_t* d_luma, int w, int h, ptrdiff_t pitch, float* d_vec) {
    if (c) c->done_armed = 0;
    if (!c || !d_luma || !d_vec) return c ? set_err(c, ETHCNN_ERR_ARG, "null pointer") : ETHCNN_ERR_ARG;
    // (FC1's epilogue stores d_vec dword by dword; the tile stage reads d_luma at any alignment, wide loads only where they fit)
    if ((uintptr_t)d_vec % 4) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_resi_vectors_device: d_vec is not 4-byte aligned");
    if (!c->have_weights) return set_err(c, ETHCNN_ERR_NOWEIGHTS, "no weights loaded");
    FrameGeom g;
    int rc = make_geom(c, w, h, pitch, (ptrdiff_t)pitch * h, &g);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    for (int o = 0; o < g.nctu; o += c->max_ctus) {
        const int n = std::min(c->max_ctus, g.nctu - o);
        rc = ensure_workspace(c, n, 1);
        if (rc) return rc;
        // one LDP frame: CTU load + trunk -> FC1 as one launch -- for a picture in HBM, and (PULL form) for a page-locked one the
        // caller is still filling (streamed input); a complete page-locked picture keeps the tile-stage launch (launch_small_pass)
        const bool streamed = c->tile_wait_rows != nullptr && c->luma_over_pcie;
        if (c->small_launch && (!c->luma_over_pcie || (streamed && c->pull)) && small_pass_ok(d_luma, g, n)) {
            // (the sync area is laid out before anything is queued: run_small_pass may wait for the stream when it has to be re-zeroed)
            rc = run_small_pass(c, d_luma, g, o, n, true, c->ws, d_vec + (size_t)o * kNVec, 0.0f, nullptr, 1, streamed, streamed ? c->tile_wait_rows : nullptr);
            if (rc) return rc;
            c->times.ctus += n;
            c->last_n = n;
    c->ws_foreign = false;
            c->last_parity = 0;
            continue;
        }
        { StageTimer t(c, ETHCNN_STAGE_TILE, n); launch_tile(d_luma, g, o, n, c->ws, 0, c->stream, 0, c->tile_wait_rows, c->rows_seq, c->h_done + 1); }
        { StageTimer t(c, ETHCNN_STAGE_TRUNK); launch_trunk(c->ws, c->dw, n, true, c->stream); }
        { StageTimer t(c, ETHCNN_STAGE_FC1, n); launch_fc1(c->ws, c->dw, n, d_vec + (size_t)o * kNVec, c->stream); }
        HIPCHK(c, hipGetLastError());
        c->times.ctus += n;
        c->last_n = n;
    c->ws_foreign = false;
        c->last_parity = 0;
    }
    return serial_end(c);
}

extern "C" int ethcnn_resi_vectors(ethcnn_ctx* c, const uint8_t* luma, int w, int h, ptrdiff_t pitch, float* vec) {
    if (!c || !luma || !vec) return c ? set_err(c, ETHCNN_ERR_ARG, "null pointer") : ETHCNN_ERR_ARG;
    if (w <= 0 || h <= 0 || pitch < w) return set_err(c, ETHCNN_ERR_ARG, "bad geometry");
    const int nctu = ((w + 63) / 64) * ((h + 63) / 64);
    const size_t lbytes = (size_t)(h - 1) * pitch + w;  // the meaningful bytes of a pitched plane: the last row ends at w
    int rc = ensure_staging(c, lbytes, (size_t)nctu * kNVec * 4);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_in[0], luma, lbytes, hipMemcpyHostToDevice, c->stream));
    rc = ethcnn_resi_vectors_device(c, c->d_in[0], w, h, pitch, c->d_out[0]);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(vec, c->d_out[0], (size_t)nctu * kNVec * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ETHCNN_OK;
}

static int ensure_lstm_buffers(ethcnn_ctx* c, int n) {
    if (n <= c->lstm_cap) return ETHCNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    void* ptrs[] = {c->d_vec, c->d_state[0], c->d_state[1], c->d_lprobs};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    c->d_vec = c->d_state[0] = c->d_state[1] = c->d_lprobs = nullptr;
    c->lstm_cap = 0;
    const int cap = (n + 15) / 16 * 16;
    HIPCHK(c, hipMalloc((void**)&c->d_vec, (size_t)cap * kNVec * 4));
    HIPCHK(c, hipMalloc((void**)&c->d_state[0], (size_t)cap * 2 * kNVec * 4));
    HIPCHK(c, hipMalloc((void**)&c->d_state[1], (size_t)cap * 2 * kNVec * 4));
    HIPCHK(c, hipMalloc((void**)&c->d_lprobs, (size_t)cap * kNOut * 4));
    c->lstm_cap = cap;
    return ETHCNN_OK;
}

// lstm() x3 + heads + gates on resident vectors: the part of sess.run after resi_cnn
// the sync area of the LSTM launch for frames of n CTUs, zeroed where it has to be (see ethcnn_lstm_step_device).  May WAIT for the
// stream (allocation, re-zeroing): a streamed step calls it before it queues kernels that wait for the caller.
static int ensure_lgate(ethcnn_ctx* c, int n) {
    const int gwords = lstm_frame_words(n);
    if (c->lgate_n != n || c->lstm_epoch >= (1 << 30)) c->lgate_clean = false;
    if (gwords > c->lgate_chunks || !c->lgate_clean) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (gwords > c->lgate_chunks) {
            if (c->d_lgate) (void)hipFree(c->d_lgate);
            c->d_lgate = nullptr;
            c->lgate_chunks = 0;
            HIPCHK(c, hipMalloc((void**)&c->d_lgate, (size_t)gwords * sizeof(int)));
            c->lgate_chunks = gwords;
        }
        HIPCHK(c, hipMemsetAsync(c->d_lgate, 0, (size_t)c->lgate_chunks * sizeof(int), c->stream));  // stream-ordered
        c->lstm_epoch = 0;
        c->lgate_n = n;
        c->lgate_clean = true;  // (zero and laid out for n: the launch below marks it dirty until it has been enqueued)
    }
    return 0;
}

extern "C" int ethcnn_lstm_step_device(ethcnn_ctx* c, const float* d_vec, const float* d_state_in, int n, int qp,
                                       int i_frame, float* d_state_out, float* d_probs) {
    if (!c || !d_vec || !d_state_out || !d_probs) return c ? set_err(c, ETHCNN_ERR_ARG, "null pointer") : ETHCNN_ERR_ARG;
    // lstm_cell reads d_vec and d_state_in as float4, the heads read d_state_out as float4 / dwordx4; d_probs is stored dword by dword
    if ((uintptr_t)d_vec % 16) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_lstm_step_device: d_vec is not 16-byte aligned");
    if ((uintptr_t)d_state_in % 16) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_lstm_step_device: d_state_in is not 16-byte aligned");
    if ((uintptr_t)d_state_out % 16) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_lstm_step_device: d_state_out is not 16-byte aligned");
    if ((uintptr_t)d_probs % 4) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_lstm_step_device: d_probs is not 4-byte aligned");
    c->done_armed = 0;
    if (n <= 0) return set_err(c, ETHCNN_ERR_ARG, "n must be positive");
    if (!c->have_lstm) return set_err(c, ETHCNN_ERR_NOWEIGHTS, "no LSTM weights loaded");
    HIPCHK(c, hipSetDevice(c->device));
    const int chunks = (n + kSubBatch - 1) / kSubBatch;
    int rc = ensure_workspace(c, std::min(n, c->max_ctus), chunks);
    if (rc) return rc;
    if (n > c->ws.cap) return set_err(c, ETHCNN_ERR_ARG, "frame of %d CTUs exceeds max_ctus_per_pass", n);
    // gate predicates + ticket tree of the LSTM heads launch: zero between launches by construction (every word is reset by its
    // last user); (re)established here after an allocation or after any failure on this path
    // (the one-launch frame kernel keeps its counters, flags and claim words behind them; a claim word holds the tag of the last
    // launch that claimed it, so the area is zeroed again whenever the frame size -- and with it the layout -- changes, and
    // before the tags wrap)
    rc = ensure_lgate(c, n);
    if (rc) return rc;
    ++c->lstm_epoch;
    c->lgate_clean = false;  // until this launch has been enqueued without an error
    const unsigned seq = done_arm(c);
    {
        StageTimer t(c, ETHCNN_STAGE_HEADS);
        launch_lstm(d_vec, d_state_in, d_state_out, c->d_lstm, n, qp, i_frame, c->thr1, c->thr2, c->debug_capture ? c->ws.raw : nullptr,
                    d_probs, c->d_lgate, seq ? c->h_done : nullptr, seq, (c->lstm_one_launch && n <= kLstmOneLaunchMaxCtus) ? 1 : 0, c->lstm_epoch, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    c->lgate_clean = true;
    c->done_armed = seq;
    c->last_n = n;
    c->ws_foreign = false;
    return serial_end(c);
}

// predict_cu_depth() of resi_to_cu_depth_LDP.py:108-129 for one frame; the new state stays in HBM.
// state source: host `state_in` when given, else zeros (resident == false) or the previous step's state in HBM.
// Two halves: ldp_step_begin enqueues everything, ldp_step_end waits and finishes the bookkeeping.  streamed: the caller is still
// FILLING the page-locked luma buffer (ethcnn_rows_ready reports its CTU rows); the tile stage waits for them row by row.
static int ldp_step_begin(ethcnn_ctx* c, const uint8_t* luma, int w, int h, ptrdiff_t pitch, int qp, int i_frame,
                          const float* state_in, bool resident, float* probs, bool streamed) {
    if (!c || !luma || !probs) return c ? set_err(c, ETHCNN_ERR_ARG, "null pointer") : ETHCNN_ERR_ARG;
    if (c->ldp.open || c->ai.open) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_step_begin: the previous streamed call has not been ended (ethcnn_ldp_step_end / ethcnn_predict_luma_end)");
    if (w <= 0 || h <= 0 || pitch < w) return set_err(c, ETHCNN_ERR_ARG, "bad geometry");
    if (!c->have_weights) return set_err(c, ETHCNN_ERR_NOWEIGHTS, "no CNN weights loaded");
    if (!c->have_lstm) return set_err(c, ETHCNN_ERR_NOWEIGHTS, "no LSTM weights loaded");
    const int nctu = ((w + 63) / 64) * ((h + 63) / 64);
    const size_t lbytes = (size_t)(h - 1) * pitch + w;  // the meaningful bytes of a pitched plane
    if (streamed) {
        if (!c->h_rows) return set_err(c, ETHCNN_ERR_DEVICE, "ethcnn_ldp_step_begin: no page-locked memory for the row words");
        if ((h + 63) / 64 > kStreamCtuRows) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_step_begin: more than %d CTU rows", kStreamCtuRows);
        if (!in_pinned(c, luma, lbytes))
            return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_step_begin: the luma buffer must come from ethcnn_host_alloc (the kernels read it in place while it is filled)");
    }
    int rc = ensure_staging(c, lbytes, (size_t)nctu * kNVec * 4);
    if (rc) return rc;
    if (nctu > c->lstm_cap) c->state_cur = -1;  // the buffers are about to be reallocated
    rc = ensure_lstm_buffers(c, nctu);
    if (rc) return rc;
    const size_t sbytes = (size_t)nctu * 2 * kNVec * 4;
    int in = -1;  // index of the input state buffer, -1 = zeros
    if (state_in) {
        in = 0;
        HIPCHK(c, hipMemcpyAsync(c->d_state[in], state_in, sbytes, hipMemcpyHostToDevice, c->stream));
    } else if (resident) {
        if (c->state_cur < 0 || c->state_nctu != nctu)
            return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_step: frame %d needs the previous frame's state, but none is resident for %d CTUs",
                           i_frame, nctu);
        in = c->state_cur;
    }
    const int out = (in == 0) ? 1 : 0;
    // Latency path (one frame, lock-step with the encoder): buffers from ethcnn_host_alloc are used IN PLACE -- the tile stage
    // reads the luma over PCIe while it runs, the heads / gate stages write the 84 B per CTU straight into the caller's
    // memory -- instead of two copy launches around the kernels
    const uint8_t* d_luma = c->d_in[0];
    // page-locked luma is read in place over PCIe by the tile stage (one coalesced pass while it runs): measured 123.8 us per
    // 1080p call against 128.3 us for "DMA it into HBM first, then the single-launch pass" (profiles/r03_latency_ldp.txt;
    // ETHCNN_LDP_INPLACE=0 selects the latter for A/B runs)
    static const bool copy_first = [] { const char* e = dev_env("ETHCNN_LDP_INPLACE"); return e && std::atoi(e) == 0; }();
    const bool in_place = in_pinned(c, luma, lbytes) && (streamed || !copy_first);
    if (in_place) d_luma = luma;
    else HIPCHK(c, hipMemcpyAsync(c->d_in[0], luma, lbytes, hipMemcpyHostToDevice, c->stream));
    const size_t pbytes = (size_t)nctu * kNOut * 4;
    // probabilities: straight into page-locked host memory (the caller's, else the staging buffer + one memcpy), the launch's
    // last block reports through the completion word
    float* d_probs = in_pinned(c, probs, pbytes) ? probs : (c->done_sync ? c->h_out[0] : c->d_lprobs);
    if (streamed) {
        // everything that may wait for the stream (allocations, re-zeroing of sync areas) happens BEFORE kernels are queued that wait
        // for the caller -- who may be this very thread, about to fill the buffer when the call returns
        HIPCHK(c, hipSetDevice(c->device));
        rc = ensure_workspace(c, std::min(nctu, c->max_ctus), (nctu + kSubBatch - 1) / kSubBatch);
        if (rc == 0) rc = ensure_lgate(c, nctu);
        if (rc) return rc;
    }
    c->luma_over_pcie = (d_luma == luma);
    c->tile_wait_rows = streamed ? c->h_rows : nullptr;
    rc = ethcnn_resi_vectors_device(c, d_luma, w, h, pitch, c->d_vec);
    c->luma_over_pcie = false;
    c->tile_wait_rows = nullptr;
    if (rc == 0) rc = ethcnn_lstm_step_device(c, c->d_vec, in >= 0 ? c->d_state[in] : nullptr, nctu, qp, i_frame, c->d_state[out], d_probs);
    if (rc) {
        // (streamed: kernels already queued may be waiting for rows the caller will now never report: release them -- the result is
        // discarded -- so that the stream drains)
        if (streamed) {
            for (int cy = 0; cy < (h + 63) / 64; ++cy) __atomic_store_n(c->h_rows + cy, c->rows_seq, __ATOMIC_RELEASE);
            (void)hipStreamSynchronize(c->stream);  // (nothing may still be reading the caller's buffer when the error is returned)
            if (++c->rows_seq == 0) c->rows_seq = 1;
        }
        return rc;
    }
    c->ldp.open = true;
    c->ldp.streamed = streamed;
    c->ldp.probs = probs;
    c->ldp.d_probs = d_probs;
    c->ldp.pbytes = pbytes;
    c->ldp.out = out;
    c->ldp.in = in;
    c->ldp.nctu = nctu;
    c->ldp.in_from_host = state_in != nullptr;
    c->ldp.prev_cur = c->state_cur;    // (after ensure_lstm_buffers: -1 when the buffers were reallocated)
    c->ldp.prev_nctu = c->state_nctu;
    return ETHCNN_OK;
}

static int ldp_step_end(ethcnn_ctx* c) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!c->ldp.open) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_step_end: no step has been begun");
    c->ldp.open = false;
    const unsigned seq = c->rows_seq;
    if (c->ldp.streamed) {  // the next streamed picture's number is fixed from here on (ethcnn_rows_ready may run before its begin)
        ++c->rows_seq;
        if (c->rows_seq == 0) c->rows_seq = 1;
    }
    if (c->ldp.d_probs == c->d_lprobs) {
        c->done_armed = 0;
        HIPCHK(c, hipMemcpyAsync(c->ldp.probs, c->d_lprobs, c->ldp.pbytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, stream_sync(c));
    if (c->ldp.streamed && __atomic_load_n(c->h_done + 1, __ATOMIC_ACQUIRE) == seq) {
        // computed on rows that never arrived: the output state is garbage, the INPUT state (the other buffer) is untouched, so the caller
        // may run the frame again (ethcnn_ldp_step on the by now complete buffer) with the same arguments.  What is resident afterwards
        // (the size must always belong to the buffer):
        //   resident input        that state, as before the step;
        //   caller's state_in     the copy of it in buffer 0, for THIS frame's CTU count;
        //   zeros (i_frame <= 1)  whatever was resident before, unless the failed step wrote over it (it wrote buffer 0).
        if (c->ldp.in_from_host) {
            c->state_cur = 0;
            c->state_nctu = c->ldp.nctu;
        } else if (c->ldp.in >= 0) {
            c->state_cur = c->ldp.in;
        } else {
            c->state_cur = (c->ldp.prev_cur == c->ldp.out) ? -1 : c->ldp.prev_cur;
            c->state_nctu = c->ldp.prev_nctu;
        }
        return set_err(c, ETHCNN_ERR_ROWS_TIMEOUT, "ethcnn_ldp_step_end: the kernels waited 1 s for luma rows that were never reported (ethcnn_rows_ready)");
    }
    if (c->ldp.d_probs == c->h_out[0]) std::memcpy(c->ldp.probs, c->ldp.d_probs, c->ldp.pbytes);
    c->state_cur = c->ldp.out;
    c->state_nctu = c->ldp.nctu;
    return ETHCNN_OK;
}

static int ldp_step_impl(ethcnn_ctx* c, const uint8_t* luma, int w, int h, ptrdiff_t pitch, int qp, int i_frame,
                         const float* state_in, bool resident, float* probs) {
    const int rc = ldp_step_begin(c, luma, w, h, pitch, qp, i_frame, state_in, resident, probs, false);
    return rc ? rc : ldp_step_end(c);
}

extern "C" int ethcnn_ldp_step(ethcnn_ctx* c, const uint8_t* luma, int w, int h, ptrdiff_t pitch, int qp, int i_frame,
                               const float* state_in, float* probs) {
    return ldp_step_impl(c, luma, w, h, pitch, qp, i_frame, state_in, /*resident=*/!state_in && i_frame > 1, probs);
}

// ---- streamed input: begin (kernels queued, waiting for rows) | rows_ready (any thread, as the buffer fills) | end
extern "C" int ethcnn_ldp_step_begin(ethcnn_ctx* c, const uint8_t* luma, int w, int h, ptrdiff_t pitch, int qp, int i_frame,
                                     const float* state_in, float* probs) {
    if (!c) return ETHCNN_ERR_ARG;
    const bool was_open = c->ai.open || c->ldp.open;
    const unsigned seq = c->rows_seq;
    const int rc = ldp_step_begin(c, luma, w, h, pitch, qp, i_frame, state_in, /*resident=*/!state_in && i_frame > 1, probs, true);
    // (a failed begin consumes the picture's number: see ethcnn_predict_luma_begin)
    if (rc != ETHCNN_OK && !was_open && c->rows_seq == seq && ++c->rows_seq == 0) c->rows_seq = 1;
    return rc;
}

extern "C" int ethcnn_rows_ready(ethcnn_ctx* c, int ctu_row_begin, int ctu_row_end) {
    // (thread-safe: touches nothing but the row words; no error text -- another thread may be inside a call on this context)
    if (!c || !c->h_rows || ctu_row_begin < 0 || ctu_row_end > kStreamCtuRows || ctu_row_begin > ctu_row_end) return ETHCNN_ERR_ARG;
    const unsigned seq = __atomic_load_n(&c->rows_seq, __ATOMIC_RELAXED);
#if defined(__SSE2__)
    _mm_sfence();  // rows written with non-temporal stores (big memcpy calls, streaming converters) are not ordered by a release store alone
#endif
    for (int cy = ctu_row_begin; cy < ctu_row_end; ++cy) __atomic_store_n(c->h_rows + cy, seq, __ATOMIC_RELEASE);
    return ETHCNN_OK;
}

extern "C" int ethcnn_ldp_step_end(ethcnn_ctx* c) { return ldp_step_end(c); }

extern "C" int ethcnn_ldp_get_state(ethcnn_ctx* c, float* state_out, size_t nfloats) {
    if (!c || !state_out) return c ? set_err(c, ETHCNN_ERR_ARG, "null pointer") : ETHCNN_ERR_ARG;
    if (c->state_cur < 0) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_get_state: no resident state (call ethcnn_ldp_step first)");
    if (nfloats != (size_t)c->state_nctu * 2 * kNVec)
        return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_get_state: the resident state holds %zu floats, not %zu", (size_t)c->state_nctu * 2 * kNVec, nfloats);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(state_out, c->d_state[c->state_cur], nfloats * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ETHCNN_OK;
}

// the reference's per-frame call as one synchronous function: state in and out through host memory
extern "C" int ethcnn_ldp_predict_frame(ethcnn_ctx* c, const uint8_t* luma, int w, int h, ptrdiff_t pitch, int qp,
                                        int i_frame, const float* state_in, float* state_out, float* probs) {
    if (!c || !luma || !state_out || !probs) return c ? set_err(c, ETHCNN_ERR_ARG, "null pointer") : ETHCNN_ERR_ARG;
    int rc = ldp_step_impl(c, luma, w, h, pitch, qp, i_frame, state_in, /*resident=*/false, probs);  // NULL = zeros here
    if (rc) return rc;
    const int nctu = ((w + 63) / 64) * ((h + 63) / 64);
    return ethcnn_ldp_get_state(c, state_out, (size_t)nctu * 2 * kNVec);
}

// ------------------------------------------------- config #5 offline: a whole residual sequence -----------
// The result of nframes successive ethcnn_ldp_step calls (frame t: i_frame = i_frame_first + t), computed the way an offline job
// should be: the front-end of a chunk of frames in the big multi-launch passes, then ONE recurrence launch per run of frames that
// carries its state on chip (ethcnn_lstm_seq.hip), then the gate post-pass.  Chunks only bound the memory: the state goes from one
// chunk to the next through the resident buffer, and the results do not depend on the chunk size (seq_chunk_frames, ethcnn_ctx.h).
extern "C" int64_t ethcnn_ldp_sequence_bytes(int w, int h, int nframes, int chunk_frames) {
    if (w <= 0 || h <= 0 || nframes <= 0 || chunk_frames < 0) return ETHCNN_ERR_ARG;
    const int64_t nctu = (int64_t)((w + 63) / 64) * ((h + 63) / 64), cap = (nctu + 15) / 16 * 16;
    const int64_t F = std::min<int64_t>(nframes, seq_chunk_frames(nctu, chunk_frames));
    // vectors + probabilities of a chunk, the two resident (c, h) buffers; no projection scratch (the recurrence runs the x half itself)
    return F * nctu * kNVec * 4 + F * nctu * kNOut * 4 + 2 * cap * 2 * kNVec * 4;
}

extern "C" int ethcnn_ldp_set_sequence_chunk(ethcnn_ctx* c, int frames) {
    if (!c) return ETHCNN_ERR_ARG;
    if (frames < 0) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_set_sequence_chunk: %d frames", frames);
    c->seq_chunk = frames;
    return ETHCNN_OK;
}

// checks shared by the three entries (nothing is allocated or enqueued before they pass); *in: the buffer that holds the state in
// front of frame 0 (-1: zeros or the caller's own)
static int seq_check(ethcnn_ctx* c, int w, int h, ptrdiff_t pitch, int64_t nframes, int i_first, bool have_state_in, int* in) {
    if (c->ldp.open || c->ai.open) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_sequence: a streamed call has not been ended");
    if (w <= 0 || h <= 0 || pitch < w) return set_err(c, ETHCNN_ERR_ARG, "bad geometry");
    if (nframes <= 0) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_sequence: nframes must be positive");
    if (i_first < 0) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_sequence: i_frame_first must not be negative");
    if (!c->have_weights) return set_err(c, ETHCNN_ERR_NOWEIGHTS, "no CNN weights loaded");
    if (!c->have_lstm) return set_err(c, ETHCNN_ERR_NOWEIGHTS, "no LSTM weights loaded");
    const int nctu = ((w + 63) / 64) * ((h + 63) / 64);
    *in = -1;
    if (i_first > 1 && !have_state_in) {
        if (c->state_cur < 0 || c->state_nctu != nctu)
            return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_step: frame %d needs the previous frame's state, but none is resident for %d CTUs", i_first, nctu);
        *in = c->state_cur;
    }
    return ETHCNN_OK;
}

// buffers of a chunk of F frames; refuses with the whole sum (ethcnn_ldp_sequence_bytes) before it allocates what it cannot get
static int seq_ensure(ethcnn_ctx* c, int w, int h, int64_t nframes, int64_t F, bool want_probs, int* in) {
    const int nctu = ((w + 63) / 64) * ((h + 63) / 64);
    const size_t vb = (size_t)F * nctu * kNVec * 4, pb = want_probs ? (size_t)F * nctu * kNOut * 4 : 0;
    HIPCHK(c, hipSetDevice(c->device));
    size_t grow = 0, back = 0;
    if (vb > c->seq_vec_cap) grow += vb, back += c->seq_vec_cap;
    if (pb > c->seq_probs_cap) grow += pb, back += c->seq_probs_cap;
    if (nctu > c->lstm_cap) grow += (size_t)((nctu + 15) / 16 * 16) * (5 * kNVec + kNOut) * 4;
    if (grow) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
        if (grow > free_b + back)
            return set_err(c, ETHCNN_ERR_NOMEM, "ethcnn_ldp_sequence: a chunk of %lld frames holds %lld bytes on the device (ethcnn_ldp_sequence_bytes); %zu are free",
                           (long long)F, (long long)ethcnn_ldp_sequence_bytes(w, h, (int)std::min<int64_t>(nframes, INT32_MAX), (int)F), free_b + back);
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (!seq_grow(&c->seq_vec, &c->seq_vec_cap, vb)) return set_err(c, ETHCNN_ERR_NOMEM, "ethcnn_ldp_sequence: %zu bytes of vectors do not fit", vb);
    if (!seq_grow(&c->seq_probs, &c->seq_probs_cap, pb)) return set_err(c, ETHCNN_ERR_NOMEM, "ethcnn_ldp_sequence: %zu bytes of probabilities do not fit", pb);
    if (nctu > c->lstm_cap) {  // (seq_check has made sure that no resident state is needed then: it belongs to another CTU count)
        c->state_cur = -1;
        *in = -1;
    }
    return ensure_lstm_buffers(c, nctu);
}

// the residual vectors of nf frames: the throughput stages ethcnn_resi_vectors_device falls back to, over passes of whole frames
int seq_front(ethcnn_ctx* c, const uint8_t* d_luma, const FrameGeom& g, int nf, float* d_vec) {
    int rc = ensure_workspace(c, (int)std::min<int64_t>((int64_t)g.nctu * nf, c->max_ctus), 1);
    if (rc) return rc;
    for (const Pass& p : plan_passes(g.nctu, nf, c->max_ctus)) {
        { StageTimer t(c, ETHCNN_STAGE_TILE, p.n); launch_tile(d_luma, g, p.ctu0, p.n, c->ws, 0, c->stream); }
        { StageTimer t(c, ETHCNN_STAGE_TRUNK); launch_trunk(c->ws, c->dw, p.n, true, c->stream); }
        { StageTimer t(c, ETHCNN_STAGE_FC1, p.n); launch_fc1(c->ws, c->dw, p.n, d_vec + (size_t)p.ctu0 * kNVec, c->stream); }
        HIPCHK(c, hipGetLastError());
        c->times.ctus += p.n;
        c->last_n = p.n;
        c->ws_foreign = false;
        c->last_parity = 0;
    }
    return ETHCNN_OK;
}

// recurrence + heads + gates of a chunk for k sequences (ethcnn_ctx.h): every row has a frame cursor; its next run is one frame if
// that frame's number is <= 0 and the rest of its chunk otherwise, with no state in front of a frame numbered <= 1.  thr1 / thr2: the
// gate pair of every row of the chunk, or null for the context's
hipError_t seq_launch(ethcnn_ctx* c, const SeqBatchRow* chunk, int k, const float* thr1, const float* thr2) {
    int at[kLstmSeqBatchMax] = {};
    for (;;) {
        SeqBatchRow rows[kLstmSeqBatchMax];
        int nr = 0;
        long ctu_frames = 0;
        for (int j = 0; j < k; ++j) {
            const SeqBatchRow& q = chunk[j];
            const int f = at[j];
            if (f >= q.F) continue;
            const int i = q.i_frame0 + f, run = (i <= 0) ? 1 : q.F - f;
            rows[nr++] = {q.vec + (size_t)f * q.n * kNVec, i <= 1 ? nullptr : (f ? q.state_out : q.state_in), q.state_out, q.blob,
                          q.probs + (size_t)f * q.n * kNOut, q.efs0, q.n, run, i};
            ctu_frames += (long)q.n * run;
            at[j] += run;
        }
        if (!nr) break;
        StageTimer t(c, ETHCNN_STAGE_HEADS, ctu_frames);
        launch_lstm_seq_batch(rows, nr, c->stream);
    }
    {
        StageTimer tg(c, ETHCNN_STAGE_GATE);
        if (thr1 && thr2) launch_lstm_seq_gates_batch(chunk, k, thr1, thr2, c->stream);
        else launch_lstm_seq_gates_batch(chunk, k, c->thr1, c->thr2, c->stream);
    }
    return hipGetLastError();
}

// the solo calls: one row on the context's bundle and the chunk's vectors in c->seq_vec; *sin: the state in front of the chunk,
// afterwards the one behind it
static int seq_launch_solo(ethcnn_ctx* c, int nctu, int nf, int qp, int i0, const float** sin, float* sout, float* d_probs) {
    const SeqBatchRow row = {c->seq_vec, *sin, sout, c->d_lstm, d_probs, lstm_seq_efs0(qp), nctu, nf, i0};
    const hipError_t e = seq_launch(c, &row, 1);
    *sin = sout;
    return e == hipSuccess ? ETHCNN_OK : set_err(c, ETHCNN_ERR_DEVICE, "hipGetLastError() failed: %s", hipGetErrorString(e));
}

extern "C" int ethcnn_ldp_sequence_device(ethcnn_ctx* c, const uint8_t* d_luma, int w, int h, ptrdiff_t pitch, ptrdiff_t fstride, int nframes,
                                          int qp, int i_first, const float* d_state_in, float* d_probs) {
    if (!c || !d_luma || !d_probs) return c ? set_err(c, ETHCNN_ERR_ARG, "null pointer") : ETHCNN_ERR_ARG;
    // lstm_seq_level reads d_state_in as float4; the recurrence and the gate pass touch d_probs dword by dword
    if ((uintptr_t)d_state_in % 16) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_sequence_device: d_state_in is not 16-byte aligned");
    if ((uintptr_t)d_probs % 4) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_sequence_device: d_probs is not 4-byte aligned");
    c->done_armed = 0;
    int in = -1;
    int rc = seq_check(c, w, h, pitch, nframes, i_first, d_state_in != nullptr, &in);
    if (rc) return rc;
    FrameGeom g;
    rc = make_geom(c, w, h, pitch, fstride, &g);
    if (rc) return rc;
    const int64_t F = std::min<int64_t>(nframes, seq_chunk_frames(g.nctu, c->seq_chunk));
    rc = seq_ensure(c, w, h, nframes, F, false, &in);
    if (rc) return rc;
    const int out = in >= 0 ? in : 0;  // the resident state is advanced in place: a block stores only its own columns (ethcnn_lstm_seq.h)
    const float* sin = i_first > 1 ? (d_state_in ? d_state_in : c->d_state[in]) : nullptr;
    c->state_cur = -1;  // until every frame has been enqueued
    for (int64_t f0 = 0; f0 < nframes; f0 += F) {
        const int nf = (int)std::min<int64_t>(F, nframes - f0);
        rc = seq_front(c, d_luma + f0 * fstride, g, nf, c->seq_vec);
        if (rc == 0) rc = seq_launch_solo(c, g.nctu, nf, qp, i_first + (int)f0, &sin, c->d_state[out], d_probs + (size_t)f0 * g.nctu * kNOut);
        if (rc) return rc;
    }
    c->state_cur = out;
    c->state_nctu = g.nctu;
    return serial_end(c);
}

// host / file entries: luma reaches the device in pieces of <= 64 MB through the context's staging ring (two of its buffers in turn),
// each piece goes through the front-end at once; the probabilities of a chunk come back through the pinned output buffer.
// fetch(dst, f, nf): frames [f, f + nf) of the sequence -> page-locked dst (null: `luma` is the caller's memory, copied from in place)
template <typename Fetch, typename Sink>
static int seq_host_run(ethcnn_ctx* c, const uint8_t* luma, int w, int h, ptrdiff_t pitch, ptrdiff_t fstride, int64_t nframes, int qp, int i_first,
                        const float* state_in, Fetch fetch, Sink sink) {
    int in = -1;
    int rc = seq_check(c, w, h, pitch, nframes, i_first, state_in != nullptr, &in);
    if (rc) return rc;
    if (fstride < (ptrdiff_t)(h - 1) * pitch + w && nframes > 1) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_sequence: frame stride %td is shorter than a frame", fstride);
    c->done_armed = 0;
    FrameGeom g;
    rc = make_geom(c, w, h, pitch, fstride, &g);
    if (rc) return rc;
    const int64_t F = std::min<int64_t>(nframes, seq_chunk_frames(g.nctu, c->seq_chunk));
    rc = seq_ensure(c, w, h, nframes, F, true, &in);
    if (rc) return rc;
    const size_t last = (size_t)(h - 1) * pitch + w;  // the meaningful bytes of the last frame of a piece
    const int pf = (int)std::max<int64_t>(1, std::min<int64_t>(F, (int64_t)(64 << 20) / std::max<int64_t>(1, (int64_t)fstride)));
    rc = ensure_staging(c, (size_t)(pf - 1) * fstride + last, (size_t)pf * g.nctu * kNOut * 4, 2);
    if (rc) return rc;
    const size_t sbytes = (size_t)g.nctu * 2 * kNVec * 4;
    const float* sin = nullptr;
    if (i_first > 1) {
        if (state_in) {
            in = 0;
            HIPCHK(c, hipMemcpyAsync(c->d_state[0], state_in, sbytes, hipMemcpyHostToDevice, c->stream));
        }
        sin = c->d_state[in];
    }
    const int out = in >= 0 ? in : 0;
    c->state_cur = -1;
    bool used[2] = {false, false};
    int piece = 0;
    // a HIP failure inside the loops leaves through the common exit below (which waits until nothing reads the caller's memory)
#define SEQCHK(call)                                                                                                   \
    {                                                                                                                  \
        const hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess) { rc = set_err(c, ETHCNN_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); break; } \
    }
    for (int64_t f0 = 0; f0 < nframes && rc == 0; f0 += F) {
        const int nf = (int)std::min<int64_t>(F, nframes - f0);
        for (int p0 = 0; p0 < nf && rc == 0; p0 += pf, ++piece) {
            const int np = std::min(pf, nf - p0), b = piece & 1;
            const size_t bytes = (size_t)(np - 1) * fstride + last;
            if (used[b]) SEQCHK(hipEventSynchronize(c->ev_in[b]));  // the piece before last has left this buffer pair
            const uint8_t* src = luma ? luma + (f0 + p0) * fstride : c->h_in[b];
            if (!luma) rc = fetch(c->h_in[b], f0 + p0, np);
            if (rc) break;
            SEQCHK(hipMemcpyAsync(c->d_in[b], src, bytes, hipMemcpyHostToDevice, c->stream));
            rc = seq_front(c, c->d_in[b], g, np, c->seq_vec + (size_t)p0 * g.nctu * kNVec);
            if (rc) break;
            SEQCHK(hipEventRecord(c->ev_in[b], c->stream));
            used[b] = true;
        }
        if (rc == 0) rc = seq_launch_solo(c, g.nctu, nf, qp, i_first + (int)f0, &sin, c->d_state[out], c->seq_probs);
        if (rc == 0) rc = sink(c->seq_probs, f0, nf, pf);
    }
#undef SEQCHK
    if (rc == 0 && hipStreamSynchronize(c->stream) != hipSuccess) rc = set_err(c, ETHCNN_ERR_DEVICE, "hipStreamSynchronize failed");
    if (rc) {
        // nothing still reads the caller's memory when the error is returned; the resident state was being advanced in place and
        // is dropped (state_cur stays -1): the next call with i_frame > 1 has to bring its state
        (void)hipStreamSynchronize(c->stream);
        c->err += " (the resident LDP state was dropped)";
        return rc;
    }
    c->state_cur = out;
    c->state_nctu = g.nctu;
    return serial_end(c);
}

extern "C" int ethcnn_ldp_sequence(ethcnn_ctx* c, const uint8_t* luma, int w, int h, ptrdiff_t pitch, ptrdiff_t fstride, int nframes, int qp,
                                   int i_first, const float* state_in, float* probs) {
    if (!c || !luma || !probs) return c ? set_err(c, ETHCNN_ERR_ARG, "null pointer") : ETHCNN_ERR_ARG;
    const size_t fb = (size_t)(w > 0 && h > 0 ? ((w + 63) / 64) * ((h + 63) / 64) : 0) * kNOut * 4;
    auto sink = [&](const float* d, int64_t f0, int nf, int) -> int {
        HIPCHK(c, hipMemcpyAsync((char*)probs + (size_t)f0 * fb, d, (size_t)nf * fb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (the next chunk overwrites d)
        return 0;
    };
    return seq_host_run(c, luma, w, h, pitch, fstride, nframes, qp, i_first, state_in, [](uint8_t*, int64_t, int) { return 0; }, sink);
}

extern "C" int ethcnn_ldp_predict_yuv_file(ethcnn_ctx* c, const char* yuv, int w, int h, int qp, const char* out_path, int64_t f_begin, int64_t f_end) {
    if (!c || !yuv || !out_path) return c ? set_err(c, ETHCNN_ERR_ARG, "null path") : ETHCNN_ERR_ARG;
    if (w <= 0 || h <= 0) return set_err(c, ETHCNN_ERR_ARG, "bad frame size %dx%d", w, h);
    struct stat st;
    if (stat(yuv, &st) != 0) return set_err(c, ETHCNN_ERR_IO, "cannot stat %s: %s", yuv, std::strerror(errno));
    const int64_t frame_bytes = (int64_t)w * h * 3 / 2;
    if (frame_bytes == 0 || st.st_size % frame_bytes != 0)
        return set_err(c, ETHCNN_ERR_FORMAT, "%s: size %lld is not a multiple of the %dx%d 4:2:0 frame size %lld", yuv, (long long)st.st_size, w, h, (long long)frame_bytes);
    const int64_t total = st.st_size / frame_bytes;
    if (f_begin == 0)  // frame k of the file is POC k (extract_data_LDP_LDB_RA.py:192 skips it as well)
        return set_err(c, ETHCNN_ERR_ARG, "ethcnn_ldp_predict_yuv_file: frame 0 is the intra picture (POC 0) and has no residual: begin at frame 1");
    if (f_begin < 0 || f_end <= f_begin || f_end > total || f_end > INT32_MAX)
        return set_err(c, ETHCNN_ERR_ARG, "frame range [%lld,%lld) outside 1..%lld", (long long)f_begin, (long long)f_end, (long long)total);
    const int nctu = ((w + 63) / 64) * ((h + 63) / 64);
    int in = -1;
    int rc = seq_check(c, w, h, w, f_end - f_begin, (int)f_begin, false, &in);  // (before any file is created)
    if (rc) return rc;
    FILE* fin = std::fopen(yuv, "rb");
    if (!fin) return set_err(c, ETHCNN_ERR_IO, "cannot open %s: %s", yuv, std::strerror(errno));
    const std::string tmp = std::string(out_path) + ".tmp." + std::to_string((long)getpid());
    FILE* fout = std::fopen(tmp.c_str(), "wb");
    if (!fout) {
        std::fclose(fin);
        return set_err(c, ETHCNN_ERR_IO, "cannot open %s for writing: %s", tmp.c_str(), std::strerror(errno));
    }
    const int fd = fileno(fin), ofd = fileno(fout);
    const size_t plane = (size_t)w * h, fb = (size_t)nctu * kNOut * 4;
    auto fetch = [&](uint8_t* dst, int64_t f, int nf) -> int {  // luma only: the chroma planes are never read
        const int bands = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(h, 32), plane / (512u << 10)));
        const std::function<int(int)> unit = [&](int u) -> int {
            const int k = u / bands, b = u % bands;
            const int r0 = (int)((long)h * b / bands), r1 = (int)((long)h * (b + 1) / bands);
            return pinned_pread(fd, dst + (size_t)k * plane + (size_t)r0 * w, (size_t)w * (r1 - r0), (off_t)(f_begin + f + k) * frame_bytes + (off_t)r0 * w);
        };
        const int r = host_pool(c)->run(nf * bands, unit);
        return r ? set_err(c, r, "short read in %s (frames %lld..%lld)", yuv, (long long)(f_begin + f), (long long)(f_begin + f + nf - 1)) : 0;
    };
    auto sink = [&](const float* d, int64_t f0, int nf, int pf) -> int {
        for (int p0 = 0; p0 < nf; p0 += pf) {
            const int np = std::min(pf, nf - p0);
            HIPCHK(c, hipMemcpyAsync(c->h_out[0], d + (size_t)p0 * nctu * kNOut, (size_t)np * fb, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            size_t done = 0;
            while (done < (size_t)np * fb) {
                const ssize_t r = pwrite(ofd, (const char*)c->h_out[0] + done, (size_t)np * fb - done, (off_t)((size_t)(f0 + p0) * fb + done));
                if (r <= 0) return set_err(c, ETHCNN_ERR_IO, "write to %s failed: %s", tmp.c_str(), std::strerror(errno));
                done += (size_t)r;
            }
        }
        return 0;
    };
    rc = seq_host_run(c, nullptr, w, h, w, (ptrdiff_t)plane, f_end - f_begin, qp, (int)f_begin, nullptr, fetch, sink);
    std::fclose(fin);
    if (std::fclose(fout) != 0 && rc == 0) rc = set_err(c, ETHCNN_ERR_IO, "close of output failed");
    if (rc == 0 && std::rename(tmp.c_str(), out_path) != 0) rc = set_err(c, ETHCNN_ERR_IO, "rename %s -> %s failed: %s", tmp.c_str(), out_path, std::strerror(errno));
    if (rc != 0) std::remove(tmp.c_str());
    return rc;
}
