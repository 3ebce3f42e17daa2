// ethcnn_ldp_sessions.cpp -- config #5 online, several live encoders (include/ethcnn.h): up to 32 sessions, each with a picture size and
// a resident state of its own, on one context; a call advances any subset of them by one frame.  A set (ethcnn_ldp_set.h) whose state
// indices are the session ids: bundles, loaders and state buffers are the set's.  The front-end is shared by the frames of a call --
// the CTU-load stage over a table of the pictures (ethcnn_tile_table.hip), then trunk and FC1 once over all 16-CTU groups --, the
// recurrence is one launch with one row of F = 1 per frame.  Frame j's result is what ethcnn_ldp_step gives on a context of its own.
#include "ethcnn_ldp_sessions_plan.h"
#include "ethcnn_ldp_set.h"

static_assert(kLdpSessionsMax == kLstmSeqBatchMax, "one row of the recurrence launch per frame of a call");
static_assert(kLdpSessionsMax <= kTileTableMax, "one table segment per frame of a call");

struct ethcnn_ldp_sessions : LdpSet {
    struct Sess {
        bool open = false;
        int w = 0, h = 0, nctu = 0;
    } q[kLdpSessionsMax];
    // ethcnn_ldp_sessions_step: the call's pictures and probabilities on the device
    float* d_stage_luma = nullptr;
    float* d_stage_probs = nullptr;
    size_t stage_luma_cap = 0, stage_probs_cap = 0;  // bytes
};

#define SCHK(s, call)                                                                                         \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) return ldp_set_err((s), ETHCNN_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

namespace {
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

int check_session(ethcnn_ldp_sessions* s, int id, const char* who) {
    if (id < 0 || id >= kLdpSessionsMax || !s->q[id].open) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: session %d is not open", who, id);
    return 0;
}

// One frame of a call behind its checks
struct Item {
    int session;
    const uint8_t* d_luma;
    FrameGeom geom;
    int qp, i_frame;
    const float* d_lstm;
    const float* d_state_in;  // the caller's state, used at ANY frame number (as ethcnn_ldp_step uses it); null: zeros (i_frame <= 1) or the resident state
    float* d_probs;
};

// The checks of both step entries: nothing is allocated or enqueued before they pass.  device: the pointers are the kernels' own.
int check_frames(ethcnn_ldp_sessions* s, const ethcnn_ldp_session_frame* frames, int n, bool device, Item* items) {
    ethcnn_ctx* c = s->c;
    const char* who = device ? "ethcnn_ldp_sessions_step_device" : "ethcnn_ldp_sessions_step";
    if (c->ldp.open || c->ai.open) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: a streamed call has not been ended", who);
    if (!c->have_weights) return ldp_set_err(s, ETHCNN_ERR_NOWEIGHTS, "no CNN weights loaded");
    if (n < 1 || n > kLdpSessionsMax) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: %d frames (1..%d)", who, n, kLdpSessionsMax);
    if (!frames) return ldp_set_err(s, ETHCNN_ERR_ARG, "null pointer");
    for (int j = 0; j < n; ++j) {
        const ethcnn_ldp_session_frame& f = frames[j];
        if (int rc = check_session(s, f.session, who)) return rc;
        for (int i = 0; i < j; ++i)
            if (frames[i].session == f.session) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: session %d is named by frames %d and %d", who, f.session, i, j);
        if (f.bundle < 0 || f.bundle >= s->nb || !s->b[f.bundle].have)
            return ldp_set_err(s, ETHCNN_ERR_NOWEIGHTS, "frame %d: bundle %d is %s (ethcnn_ldp_sessions_load_lstm_*)", j, f.bundle,
                               f.bundle < 0 || f.bundle >= s->nb ? "outside the object's bundles" : "empty");
        if (!f.luma || !f.probs) return ldp_set_err(s, ETHCNN_ERR_ARG, "null pointer (frame %d)", j);
        // lstm_seq_level reads a state as float4; probs is touched dword by dword
        if (device && (uintptr_t)f.state_in % 16) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: state_in of frame %d is not 16-byte aligned", who, j);
        if (device && (uintptr_t)f.probs % 4) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: probs of frame %d is not 4-byte aligned", who, j);
        const ethcnn_ldp_sessions::Sess& q = s->q[f.session];
        if (f.pitch < q.w) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: pitch %td < width %d (frame %d)", who, f.pitch, q.w, j);
        FrameGeom geom;
        if (int rc = make_geom(c, q.w, q.h, f.pitch, (ptrdiff_t)f.pitch * q.h, &geom)) return ldp_set_err(s, rc, "frame %d: %s", j, c->err.c_str());
        if (f.i_frame > 1 && !f.state_in && s->s[f.session].state_nctu != geom.nctu)
            return ldp_set_err(s, ETHCNN_ERR_ARG, "ethcnn_ldp_step: frame %d needs the previous frame's state, but none is resident for %d CTUs (session %d)",
                               f.i_frame, geom.nctu, f.session);
        items[j] = {f.session, f.luma, geom, f.qp, f.i_frame, s->b[f.bundle].d_lstm, f.state_in, f.probs};
    }
    // probs against every buffer of the call that a kernel still reads while the heads and the gate pass write it: the other frames'
    // probs, every frame's state_in (its own included) and every frame's picture
    for (int j = 0; j < n; ++j) {
        const size_t pj = (size_t)items[j].geom.nctu * kNOut * 4;
        for (int i = 0; i < n; ++i) {
            const FrameGeom& g = items[i].geom;
            if ((i != j && overlap(items[j].d_probs, pj, items[i].d_probs, (size_t)g.nctu * kNOut * 4)) ||
                (items[i].d_state_in && overlap(items[j].d_probs, pj, items[i].d_state_in, (size_t)g.nctu * kLdpStateFloats * 4)) ||
                overlap(items[j].d_probs, pj, items[i].d_luma, (size_t)(g.height - 1) * g.pitch + g.width))
                return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: probs of frame %d overlaps a buffer of frame %d", who, j, i);
        }
    }
    return ETHCNN_OK;
}

void drop_states(ethcnn_ldp_sessions* s, const Item* items, int n) {
    for (int j = 0; j < n; ++j) s->s[items[j].session].state_nctu = -1;
}

struct Layout {
    int first[kLdpSessionsMax], gpp;
    int64_t groups;
};

// Behind the checks, in front of anything that touches a state: the layout of the call and its vector buffer
int sessions_buffers(ethcnn_ldp_sessions* s, const Item* items, int n, const char* who, Layout* L) {
    ethcnn_ctx* c = s->c;
    int nctus[kLdpSessionsMax];
    for (int j = 0; j < n; ++j) nctus[j] = items[j].geom.nctu;
    if (ldp_sessions_layout(nctus, n, c->max_ctus, L->first, &L->groups, &L->gpp)) return ldp_set_err(s, ETHCNN_ERR_ARG, "%s: too many CTUs in one call", who);
    const size_t vb = (size_t)L->groups * 16 * kNVec * 4;  // every picture's slice starts at a multiple of 16 rows
    SCHK(s, hipSetDevice(c->device));
    if (vb > s->vec_cap) {
        size_t free_b = 0, total_b = 0;
        SCHK(s, hipMemGetInfo(&free_b, &total_b));
        if (vb > free_b + s->vec_cap)
            return ldp_set_err(s, ETHCNN_ERR_NOMEM, "%s: %d frames hold %zu bytes of vectors on the device (ethcnn_ldp_sessions_bytes); %zu are free", who, n, vb,
                               free_b + s->vec_cap);
        SCHK(s, hipStreamSynchronize(c->stream));
        if (!seq_grow(&s->d_vec, &s->vec_cap, vb)) return ldp_set_err(s, ETHCNN_ERR_NOMEM, "%s: %zu bytes of vectors do not fit", who, vb);
    }
    return ETHCNN_OK;
}

// The shared front-end, one recurrence and one gate launch.  A failure in here drops the states of the call's sessions (they are
// advanced in place).
int sessions_launch(ethcnn_ldp_sessions* s, const Item* items, int n, const Layout& L) {
    ethcnn_ctx* c = s->c;
    const int* const first = L.first;
    const int64_t groups = L.groups;
    const int gpp = L.gpp;
    if (int rc = ensure_workspace(c, (int)std::min<int64_t>(groups, gpp) * 16, 1)) {
        drop_states(s, items, n);
        return ldp_set_err(s, rc, "%s (the resident states of the call's sessions were dropped)", c->err.c_str());
    }
    c->done_armed = 0;
    drop_states(s, items, n);  // until everything has been enqueued
#ifdef ETHCNN_EXPERIMENTS
    // A/B switch of scripts/ldp_sessions_rate.py: the front-end per picture, as the offline batch runs it (3 launches per frame)
    static const bool solo_front = [] { const char* e = dev_env("ETHCNN_SESSIONS_FRONT"); return e && std::strcmp(e, "solo") == 0; }();
#else
    constexpr bool solo_front = false;
#endif
    if (solo_front) {
        for (int j = 0; j < n; ++j)
            if (int rc = seq_front(c, items[j].d_luma, items[j].geom, 1, s->d_vec + (size_t)first[j] * 16 * kNVec))
                return ldp_set_err(s, rc, "frame %d: %s (the resident states of the call's sessions were dropped)", j, c->err.c_str());
    } else {
        TileTable tab;
        std::memset(&tab, 0, sizeof tab);
        tab.nseg = n;
        for (int j = 0; j < n; ++j) tab.seg[j] = tile_seg(items[j].d_luma, items[j].geom, items[j].geom.nctu, first[j]);
        for (int64_t g0 = 0; g0 < groups; g0 += gpp) {
            const int ng = (int)std::min<int64_t>(gpp, groups - g0), rows = ng * 16;
            { StageTimer t(c, ETHCNN_STAGE_TILE, rows); launch_tile_table(tab, (int)g0, ng, c->ws, c->stream); }
            { StageTimer t(c, ETHCNN_STAGE_TRUNK); launch_trunk(c->ws, c->dw, rows, true, c->stream); }
            { StageTimer t(c, ETHCNN_STAGE_FC1, rows); launch_fc1(c->ws, c->dw, rows, s->d_vec + (size_t)g0 * 16 * kNVec, c->stream); }
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess)
                return ldp_set_err(s, ETHCNN_ERR_DEVICE, "launch failed: %s (the resident states of the call's sessions were dropped)", hipGetErrorString(e));
            c->times.ctus += rows;
            c->last_n = rows;
            c->ws_foreign = false;
            c->last_parity = 0;
        }
    }
    // One row of one frame per session.  The state rule is ethcnn_ldp_step's: the caller's state at any frame number, else zeros in
    // front of a frame numbered <= 1, else the resident state.  Every row is one run, so the two launchers are called as they are:
    // seq_launch (ethcnn_ldp.cpp) would zero the state in front of EVERY frame numbered <= 1, the offline calls' rule.
    SeqBatchRow rows[kLdpSessionsMax];
    float thr1[kLdpSessionsMax], thr2[kLdpSessionsMax];  // by row: the pair follows the session id, not the row position
    long ctu_frames = 0;
    for (int j = 0; j < n; ++j) {
        const Item& it = items[j];
        ldp_set_gates_of(s, it.session, &thr1[j], &thr2[j]);
        float* const state = s->s[it.session].d_state;
        rows[j] = {s->d_vec + (size_t)first[j] * 16 * kNVec, it.d_state_in ? it.d_state_in : (it.i_frame > 1 ? state : nullptr), state, it.d_lstm, it.d_probs,
                   lstm_seq_efs0(it.qp), it.geom.nctu, 1, it.i_frame};
        ctu_frames += it.geom.nctu;
    }
    { StageTimer t(c, ETHCNN_STAGE_HEADS, ctu_frames); launch_lstm_seq_batch(rows, n, c->stream); }
    { StageTimer t(c, ETHCNN_STAGE_GATE); launch_lstm_seq_gates_batch(rows, n, thr1, thr2, c->stream); }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return ldp_set_err(s, ETHCNN_ERR_DEVICE, "launch failed: %s (the resident states of the call's sessions were dropped)", hipGetErrorString(e));
    for (int j = 0; j < n; ++j) s->s[items[j].session].state_nctu = items[j].geom.nctu;
    const int rc = serial_end(c);
    return rc ? ldp_set_err(s, rc, "%s", c->err.c_str()) : ETHCNN_OK;
}
}  // namespace

extern "C" int ethcnn_ldp_sessions_create(ethcnn_ctx* c, int nbundles, ethcnn_ldp_sessions** out) {
    return ldp_set_create(c, nbundles, kLdpSessionsMax, "ethcnn_ldp_sessions_create", "bundles", out);
}
extern "C" void ethcnn_ldp_sessions_destroy(ethcnn_ldp_sessions* s) {
    if (!s) return;
    ldp_set_release(s);  // (waits for the stream)
    if (s->d_stage_luma) (void)hipFree(s->d_stage_luma);
    if (s->d_stage_probs) (void)hipFree(s->d_stage_probs);
    delete s;
}
extern "C" const char* ethcnn_ldp_sessions_last_error(const ethcnn_ldp_sessions* s) { return s ? s->err.c_str() : "LDP sessions object is NULL"; }
extern "C" int ethcnn_ldp_sessions_bundles(const ethcnn_ldp_sessions* s) { return s ? s->nb : ETHCNN_ERR_ARG; }
extern "C" int ethcnn_ldp_sessions_load_lstm_blob(ethcnn_ldp_sessions* s, int i, const float* blob, size_t nfloats) {
    return ldp_set_load_blob(s, i, blob, nfloats, "ethcnn_ldp_sessions_load_lstm_blob", "bundle");
}
extern "C" int ethcnn_ldp_sessions_load_lstm_synthetic(ethcnn_ldp_sessions* s, int i, uint64_t seed, double head_gain) {
    return ldp_set_load_synthetic(s, i, seed, head_gain, "ethcnn_ldp_sessions_load_lstm_synthetic", "bundle");
}
extern "C" int ethcnn_ldp_sessions_load_lstm_checkpoint(ethcnn_ldp_sessions* s, int i, const char* prefix) {
    return ldp_set_load_checkpoint(s, i, prefix, "ethcnn_ldp_sessions_load_lstm_checkpoint", "bundle");
}
extern "C" int ethcnn_ldp_sessions_get_lstm_blob(ethcnn_ldp_sessions* s, int i, float* out, size_t nfloats) {
    return ldp_set_get_blob(s, i, out, nfloats, "ethcnn_ldp_sessions_get_lstm_blob", "bundle");
}

extern "C" int ethcnn_ldp_sessions_open(ethcnn_ldp_sessions* s, int width, int height, int* session) {
    if (!s) return ETHCNN_ERR_ARG;
    if (!session) return ldp_set_err(s, ETHCNN_ERR_ARG, "null pointer");
    *session = -1;
    if (width <= 0 || height <= 0) return ldp_set_err(s, ETHCNN_ERR_ARG, "ethcnn_ldp_sessions_open: bad frame size %dx%d", width, height);
    int id = 0;
    while (id < kLdpSessionsMax && s->q[id].open) ++id;
    if (id == kLdpSessionsMax) return ldp_set_err(s, ETHCNN_ERR_ARG, "ethcnn_ldp_sessions_open: %d sessions are open already", kLdpSessionsMax);
    const int64_t nctu = (((int64_t)width + 63) / 64) * (((int64_t)height + 63) / 64);
    if (nctu > INT32_MAX / 16) return ldp_set_err(s, ETHCNN_ERR_ARG, "ethcnn_ldp_sessions_open: bad frame size %dx%d", width, height);
    LdpSet::State& S = s->s[id];
    S.state_nctu = -1;
    if (nctu > S.cap) {
        ethcnn_ctx* c = s->c;
        const size_t bytes = (size_t)((nctu + 15) / 16 * 16 * kLdpStateFloats * 4);
        SCHK(s, hipSetDevice(c->device));
        SCHK(s, hipStreamSynchronize(c->stream));  // (a closed session's last step may still be using the buffer)
        size_t held = 0;
        S.cap = 0;
        if (!seq_grow(&S.d_state, &held, bytes)) return ldp_set_err(s, ETHCNN_ERR_NOMEM, "ethcnn_ldp_sessions_open: %zu bytes of state do not fit", bytes);
        S.cap = (int)((nctu + 15) / 16 * 16);
    }
    s->q[id] = {true, width, height, (int)nctu};
    *session = id;
    return ETHCNN_OK;
}

extern "C" int ethcnn_ldp_sessions_close(ethcnn_ldp_sessions* s, int session) {
    if (!s) return ETHCNN_ERR_ARG;
    if (int rc = check_session(s, session, "ethcnn_ldp_sessions_close")) return rc;
    s->q[session] = {};
    s->s[session].state_nctu = -1;  // (the buffer stays for the next session of this id)
    s->s[session].own_gates = false;  // (a reused id starts by inheriting the context's pair)
    return ETHCNN_OK;
}

extern "C" int ethcnn_ldp_sessions_set_thresholds(ethcnn_ldp_sessions* s, int session, float thr_l1_lower, float thr_l2_lower) {
    if (!s) return ETHCNN_ERR_ARG;
    if (int rc = check_session(s, session, "ethcnn_ldp_sessions_set_thresholds")) return rc;
    return ldp_set_set_gates(s, session, thr_l1_lower, thr_l2_lower, "ethcnn_ldp_sessions_set_thresholds", "session");
}
extern "C" int ethcnn_ldp_sessions_clear_thresholds(ethcnn_ldp_sessions* s, int session) {
    if (!s) return ETHCNN_ERR_ARG;
    if (int rc = check_session(s, session, "ethcnn_ldp_sessions_clear_thresholds")) return rc;
    return ldp_set_clear_gates(s, session, "ethcnn_ldp_sessions_clear_thresholds", "session");
}
extern "C" int ethcnn_ldp_sessions_get_thresholds(ethcnn_ldp_sessions* s, int session, float* thr_l1_lower, float* thr_l2_lower, int* own) {
    if (!s) return ETHCNN_ERR_ARG;
    if (int rc = check_session(s, session, "ethcnn_ldp_sessions_get_thresholds")) return rc;
    return ldp_set_get_gates(s, session, thr_l1_lower, thr_l2_lower, own, "ethcnn_ldp_sessions_get_thresholds", "session");
}

extern "C" int64_t ethcnn_ldp_sessions_state_ctus(ethcnn_ldp_sessions* s, int session) {
    if (!s) return ETHCNN_ERR_ARG;
    if (int rc = check_session(s, session, "ethcnn_ldp_sessions_state_ctus")) return rc;
    return ldp_set_state_ctus(s, session, "ethcnn_ldp_sessions_state_ctus", "session");
}

extern "C" int ethcnn_ldp_sessions_get_state(ethcnn_ldp_sessions* s, int session, float* out, size_t nfloats) {
    if (!s) return ETHCNN_ERR_ARG;
    if (int rc = check_session(s, session, "ethcnn_ldp_sessions_get_state")) return rc;
    return ldp_set_get_state(s, session, out, nfloats, "ethcnn_ldp_sessions_get_state", "session");
}

extern "C" int ethcnn_ldp_sessions_step_device(ethcnn_ldp_sessions* s, const ethcnn_ldp_session_frame* frames, int n) {
    if (!s) return ETHCNN_ERR_ARG;
    Item items[kLdpSessionsMax];
    if (int rc = check_frames(s, frames, n, true, items)) return rc;
    Layout L;
    if (int rc = sessions_buffers(s, items, n, "ethcnn_ldp_sessions_step_device", &L)) return rc;
    return sessions_launch(s, items, n, L);
}

extern "C" int ethcnn_ldp_sessions_step(ethcnn_ldp_sessions* s, const ethcnn_ldp_session_frame* frames, int n) {
    if (!s) return ETHCNN_ERR_ARG;
    Item items[kLdpSessionsMax];
    if (int rc = check_frames(s, frames, n, false, items)) return rc;
    ethcnn_ctx* c = s->c;
    // the pictures (each at a 256-byte boundary, its pitch kept) and the probabilities of the call on the device
    size_t loff[kLdpSessionsMax + 1], poff[kLdpSessionsMax + 1];
    loff[0] = poff[0] = 0;
    for (int j = 0; j < n; ++j) {
        const FrameGeom& g = items[j].geom;
        loff[j + 1] = loff[j] + ((size_t)(g.height - 1) * g.pitch + g.width + 255) / 256 * 256;
        poff[j + 1] = poff[j] + (size_t)g.nctu * kNOut * 4;
    }
    SCHK(s, hipSetDevice(c->device));
    if (loff[n] > s->stage_luma_cap || poff[n] > s->stage_probs_cap) {
        SCHK(s, hipStreamSynchronize(c->stream));
        if (!seq_grow(&s->d_stage_luma, &s->stage_luma_cap, loff[n]) || !seq_grow(&s->d_stage_probs, &s->stage_probs_cap, poff[n]))
            return ldp_set_err(s, ETHCNN_ERR_NOMEM, "ethcnn_ldp_sessions_step: %zu bytes of pictures and probabilities do not fit", loff[n] + poff[n]);
    }
    Layout L;
    int rc = sessions_buffers(s, items, n, "ethcnn_ldp_sessions_step", &L);
    if (rc) return rc;
    // every refusal that keeps the states lies in front of this line: a caller's state goes into the session's own buffer
    hipError_t e = hipSuccess;
    for (int j = 0; j < n && e == hipSuccess; ++j) {
        Item& it = items[j];
        const FrameGeom& g = it.geom;
        uint8_t* const d_luma = (uint8_t*)s->d_stage_luma + loff[j];
        e = hipMemcpyAsync(d_luma, it.d_luma, (size_t)(g.height - 1) * g.pitch + g.width, hipMemcpyHostToDevice, c->stream);
        it.d_luma = d_luma;
        if (it.d_state_in && e == hipSuccess) {  // into the session's own buffer: the step advances it in place
            float* const state = s->s[it.session].d_state;
            s->s[it.session].state_nctu = -1;
            e = hipMemcpyAsync(state, it.d_state_in, (size_t)g.nctu * kLdpStateFloats * 4, hipMemcpyHostToDevice, c->stream);
            it.d_state_in = state;
        }
    }
    float* host_probs[kLdpSessionsMax];
    for (int j = 0; j < n; ++j) host_probs[j] = items[j].d_probs, items[j].d_probs = (float*)((char*)s->d_stage_probs + poff[j]);
    if (e == hipSuccess) rc = sessions_launch(s, items, n, L);
    for (int j = 0; j < n && e == hipSuccess && rc == ETHCNN_OK; ++j)
        e = hipMemcpyAsync(host_probs[j], items[j].d_probs, poff[j + 1] - poff[j], hipMemcpyDeviceToHost, c->stream);
    // nothing still reads or writes the caller's memory when the call returns
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        drop_states(s, items, n);
        return ldp_set_err(s, ETHCNN_ERR_DEVICE, "ethcnn_ldp_sessions_step: %s (the resident states of the call's sessions were dropped)", hipGetErrorString(e));
    }
    return rc;
}
