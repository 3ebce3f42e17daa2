// ethcnn_ldp_set.h -- internal: the one object behind ethcnn_ldp_group_* and ethcnn_ldp_batch_* (include/ethcnn.h "config #5
// offline", group and batch form) and the one run behind their device entries.  Several sequences go through the offline
// Low-Delay-P chain together: the front-end per sequence (seq_front into the sequence's slice of the vector buffer), then the
// recurrence and gate launches of a chunk for all sequences that still have frames (seq_launch, ethcnn_ctx.h).  A group is a batch
// of K rows of one geometry, length and first frame number in which sequence m uses bundle m.  Bundles are held apart from the
// sequences: several sequences of one QP band name the same image.  The context's own bundle, resident state and sequence buffers
// are neither used nor changed.  ethcnn_ldp_sessions (ethcnn_ldp_sessions.cpp, the online form) is a set as well: its state indices are
// session ids, and it has a run of its own (one frame per session through a shared front-end).
#pragma once
#include "ethcnn_ctx.h"
#include "ethcnn_lstm_seq.h"

constexpr int kLdpSetBundles = 8;
static_assert(kLdpSetBundles == kLstmSeqGroupMax, "a group holds one bundle per member");

struct LdpSet {
    ethcnn_ctx* c = nullptr;
    int nb = 0;       // bundles (a group: its members)
    int nstates = 0;  // state indices a caller may name: a group's members, a batch's kLstmSeqBatchMax
    int chunk = 0;    // frames per chunk, 0 = default (256 MB of vectors for all sequences of the call)
    std::string err;
    struct Bundle {
        bool have = false;
        std::vector<float> blob;  // the payload as stored
        float* d_lstm = nullptr;  // payload + packed kernels in HBM (upload_lstm_image), held from load time
    } b[kLdpSetBundles];
    struct State {
        float* d_state = nullptr;  // the resident (c, h) state of this sequence index, [cap][2][448], advanced in place
        int cap = 0;               // CTUs, a multiple of 16
        int state_nctu = -1;       // CTU count of the resident state; -1: none
        bool own_gates = false;    // thr1, thr2 below are this index's gate pair; else it inherits the context's at launch time
        float thr1 = 0.f, thr2 = 0.f;
    } s[kLstmSeqBatchMax];
    float* d_vec = nullptr;  // the chunk's vectors, sequence after sequence: [min(nframes_j, Fc)][nctu_j][448]
    size_t vec_cap = 0;      // bytes
};
struct ethcnn_ldp_group : LdpSet {};
struct ethcnn_ldp_batch : LdpSet {};

constexpr int64_t kLdpStateFloats = 2 * kNVec;  // (c, h) of a CTU

// An entry passes the words that differ between the forms, so that every message keeps its wording: who (the entry's name) and
// what ("member", "bundle" or "sequence index": what the entry calls index i).  A null set is ETHCNN_ERR_ARG in all of them.
int ldp_set_err(LdpSet* s, int code, const char* fmt, ...);
int ldp_set_load_blob(LdpSet* s, int i, const float* blob, size_t nfloats, const char* who, const char* what);
int ldp_set_load_synthetic(LdpSet* s, int i, uint64_t seed, double head_gain, const char* who, const char* what);
int ldp_set_load_checkpoint(LdpSet* s, int i, const char* prefix, const char* who, const char* what);
int ldp_set_get_blob(LdpSet* s, int i, float* out, size_t nfloats, const char* who, const char* what);
int ldp_set_chunk(LdpSet* s, int frames, const char* who);
int64_t ldp_set_state_ctus(LdpSet* s, int j, const char* who, const char* what);
int ldp_set_get_state(LdpSet* s, int j, float* out, size_t nfloats, const char* who, const char* what);
// The gate pair of a state index (host-only bookkeeping, nothing touches the stream; refused while a streamed call is open).  Values as
// ethcnn_set_thresholds takes them: that entry refuses no float, so neither do these.  get: own_out says whether the pair is the
// index's own or the context's as it stands now; every output pointer is needed.
int ldp_set_set_gates(LdpSet* s, int j, float thr1, float thr2, const char* who, const char* what);
int ldp_set_clear_gates(LdpSet* s, int j, const char* who, const char* what);
int ldp_set_get_gates(LdpSet* s, int j, float* thr1, float* thr2, int* own_out, const char* who, const char* what);
// the pair state index j runs under in a launch enqueued now: its own if set, else the context's thr1 / thr2 read at this call
inline void ldp_set_gates_of(const LdpSet* s, int j, float* thr1, float* thr2) {
    const LdpSet::State& S = s->s[j];
    *thr1 = S.own_gates ? S.thr1 : s->c->thr1;
    *thr2 = S.own_gates ? S.thr2 : s->c->thr2;
}
void ldp_set_release(LdpSet* s);  // waits for the stream and frees what the set holds on the device (the entry deletes the object)

template <class T>  // T: ethcnn_ldp_group or ethcnn_ldp_batch; what: "members" or "bundles"
int ldp_set_create(ethcnn_ctx* c, int nb, int nstates, const char* who, const char* what, T** out) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "null output pointer");
    *out = nullptr;
    if (nb < 1 || nb > kLdpSetBundles) return set_err(c, ETHCNN_ERR_ARG, "%s: %d %s (1..%d)", who, nb, what, kLdpSetBundles);
    T* s = new (std::nothrow) T;
    if (!s) return set_err(c, ETHCNN_ERR_NOMEM, "out of memory");
    s->c = c;
    s->nb = nb;
    s->nstates = nstates;
    *out = s;
    return ETHCNN_OK;
}

// One sequence of a run, checked by its entry.  Sequence j of the call uses the resident state of index j.
struct LdpSeq {
    const uint8_t* d_luma;
    FrameGeom geom;
    int nframes, i_frame_first, qp;
    const float* d_lstm;      // its bundle's image
    const float* d_state_in;  // the caller's state in front of the first frame; null: the resident one (zeros up to frame 1)
    float* d_probs;
};
// The part of ethcnn_ldp_group_sequence_device and ethcnn_ldp_batch_run_device behind their checks, from "buffers" onward: chunk
// size, the memory sum and its refusal, the vector and state buffers, the workspace, then per chunk the front-end of every sequence
// that has frames left and seq_launch.  who: the entry's name without "_device"; item: "member" or "sequence"; form: "group" or
// "batch".
int ldp_set_run(LdpSet* s, const LdpSeq* seqs, int nseqs, const char* who, const char* item, const char* form);
