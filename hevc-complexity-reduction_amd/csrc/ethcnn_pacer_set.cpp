// ethcnn_pacer_set.cpp -- host side of the pacer set (include/ethcnn.h "search budget, online: several sequences"): up to 32 slots, each
// what a solo pacer (ethcnn_pacer.cpp) keeps per sequence and bound to one of up to 32 POLICIES {ladder, weights, budget, mode}; a call over n
// frames is k_pacer_table and k_pacer_bake_table (ethcnn_pacer_set.hip), two launches on the context's stream whatever n is and whatever
// policies its slots have.  ethcnn_pacer_set_create makes a set of one policy bound to every slot.
#include "ethcnn_analysis.h"
#include "ethcnn_budget.h"
#include "ethcnn_pacer_set.h"

using namespace ethcnn::pacer;
using ethcnn::budget::kNout;

struct ethcnn_pacer_set {
    ethcnn_ctx* c = nullptr;
    int nslots = 0;
    int npolicies = 0;
    PolicyRec policy[kPacerSetMaxPolicies] = {};  // (set by create; the device holds a copy)
    int slot_policy[kPacerSetMax] = {};
    int stride = 0;                 // the most rungs of any policy: rows of a slot's table
    int* d_thr = nullptr;           // [sum of rungs][6]: every policy's ladder, then its full search
    PolicyRec* d_policy = nullptr;  // [npolicies]
    unsigned* d_checked = nullptr;  // [nslots][stride][4]
    unsigned* d_state = nullptr;    // [nslots][kStateWords]
    unsigned* d_recs = nullptr;     // record scratch of a call, 64 bytes a CTU
    int64_t cap_recs = 0;           // in CTUs
    float* d_stage = nullptr;       // staging of the host form for pageable pointers, 84 bytes a CTU
    int64_t cap_stage = 0;
    ethcnn_pacer_result* h_result = nullptr;  // [nslots], page-locked
    int64_t queued[kPacerSetMax] = {};        // frames enqueued per slot since create / reset
    int64_t launches = 0;                     // kernels enqueued since create
};

namespace {
struct Checked {
    int64_t per[kPacerSetMax], K[kPacerSetMax];
    PacerSetSeg seg[kPacerSetMax];
    int64_t total, count_grid, bake_grid;
};

// every refusal of a call, before anything is allocated or enqueued; device: `result` is a device pointer (4-byte aligned) too
int check_call(ethcnn_pacer_set* p, const ethcnn_pacer_set_frame* f, int n, bool device, Checked* k) {
    ethcnn_ctx* c = p->c;
    if (n < 1 || n > kPacerSetMax) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set: %d frames in a call (1..%d)", n, kPacerSetMax);
    if (!f) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set: null frames");
    int named[kPacerSetMax];
    for (int s = 0; s < kPacerSetMax; ++s) named[s] = -1;
    for (int j = 0; j < n; ++j) {
        if (f[j].slot < 0 || f[j].slot >= p->nslots) return set_err(c, ETHCNN_ERR_ARG, "frame %d: slot %d is outside 0..%d", j, f[j].slot, p->nslots - 1);
        if (named[f[j].slot] >= 0) return set_err(c, ETHCNN_ERR_ARG, "slot %d is named by frames %d and %d", f[j].slot, named[f[j].slot], j);
        named[f[j].slot] = j;
        if (!f[j].probs || !f[j].baked) return set_err(c, ETHCNN_ERR_ARG, "frame %d: null probabilities or output buffer", j);
        if ((uintptr_t)f[j].probs % 4 || (uintptr_t)f[j].baked % 4 || (device && (uintptr_t)f[j].result % 4))
            return set_err(c, ETHCNN_ERR_ARG, "frame %d: a pointer is not 4-byte aligned", j);
        const PolicyRec& pr = p->policy[p->slot_policy[f[j].slot]];
        const uint64_t weight[4] = {pr.weight[0], pr.weight[1], pr.weight[2], pr.weight[3]};
        if (int rc = check_frame(c, weight, f[j].width, f[j].height, &k->per[j])) return rc;  // (the bound under the weights of ITS slot's policy)
        k->K[j] = pr.rungs - 1;
    }
    // an output may be its own frame's input (in place); it may not touch another frame's input or output
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (i == j) continue;
            const uintptr_t b = (uintptr_t)f[i].baked, be = b + (uintptr_t)k->per[i] * kNout * 4, bytes = (uintptr_t)k->per[j] * kNout * 4;
            const uintptr_t q = (uintptr_t)f[j].probs, o = (uintptr_t)f[j].baked;
            if ((b < q + bytes && q < be) || (i < j && b < o + bytes && o < be))
                return set_err(c, ETHCNN_ERR_ARG, "the output of frame %d overlaps a buffer of frame %d", i, j);
        }
    if (pacer_set_layout_rungs(k->per, k->K, n, k->seg, &k->count_grid, &k->bake_grid))
        return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set: no layout for these frames");  // (every rule was checked above)
    k->total = k->seg[n - 1].rec0 + k->per[n - 1];
    return 0;
}

// checked arguments, device-addressable pointers: the two launches
int enqueue(ethcnn_pacer_set* p, const ethcnn_pacer_set_frame* f, int n, const Checked& k) {
    ethcnn_ctx* c = p->c;
    c->done_armed = 0;  // the context's completion word does not cover these launches
    FrameTable t;
    BakeTable b;
    t.nseg = b.nseg = n;
    t.stride = p->stride;
    t.policy = p->d_policy;
    t.one = p->policy[0];
    t.thr = p->d_thr;
    t.checked = p->d_checked;
    t.state = p->d_state;
    t.recs = p->d_recs;
    t.h_result = p->h_result;
    b.recs = p->d_recs;
    b.state = p->d_state;
    for (int j = 0; j < n; ++j) {
        const PacerSetSeg& s = k.seg[j];
        t.seg[j] = TableSeg{f[j].probs, f[j].result, (long)s.rec0, f[j].width, f[j].height, (f[j].width + 63) / 64, (int)k.per[j],
                            (int)s.count_first, (int)s.count_blocks, s.slice_len, f[j].slot, p->slot_policy[f[j].slot],
                            (int)((k.K[j] + 1 + kPacerSetThreads - 1) / kPacerSetThreads)};
        b.seg[j] = BakeSeg{reinterpret_cast<unsigned*>(f[j].baked), (long)s.rec0, (int)k.per[j], (int)s.bake_first, f[j].slot, 0};
    }
    for (int j = n; j < kPacerSetMax; ++j) t.seg[j] = TableSeg{}, b.seg[j] = BakeSeg{};
    (void)hipGetLastError();
    launch_table(c->stream, t, (unsigned)k.count_grid, p->npolicies > 1);
    launch_bake_table(c->stream, b, (unsigned)k.bake_grid);
    HIPCHK(c, hipGetLastError());
    p->launches += 2;
    for (int j = 0; j < n; ++j) ++p->queued[f[j].slot];
    return 0;
}
}  // namespace

// the rules of a policy list and of a binding; c may be NULL (the message then goes where ethcnn_last_error(NULL) reads)
static int check_policies(ethcnn_ctx* c, const ethcnn_pacer_policy* policies, int npolicies, const int* slot_policy, int nslots) {
    if (npolicies < 1 || npolicies > kPacerSetMaxPolicies) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set: %d policies (1..%d)", npolicies, kPacerSetMaxPolicies);
    if (!policies) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set: null policies");
    if (nslots < 0 || nslots > kPacerSetMax) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set: %d slots (1..%d)", nslots, kPacerSetMax);
    for (int i = 0; i < npolicies; ++i) {
        const ethcnn_pacer_policy& q = policies[i];
        if (check_rules(c, q.ladder, q.K, q.weight, q.budget_ppm, q.mode)) {
            const std::string why = ethcnn_last_error(c);
            return set_err(c, ETHCNN_ERR_ARG, "policy %d: %s", i, why.c_str());
        }
    }
    if (slot_policy)
        for (int s = 0; s < nslots; ++s)
            if (slot_policy[s] < 0 || slot_policy[s] >= npolicies)
                return set_err(c, ETHCNN_ERR_ARG, "slot %d: policy %d is outside 0..%d", s, slot_policy[s], npolicies - 1);
    return 0;
}

extern "C" int ethcnn_pacer_policies_check(const ethcnn_pacer_policy* policies, int npolicies, const int* slot_policy, int nslots) {
    return check_policies(nullptr, policies, npolicies, slot_policy, nslots);
}

extern "C" int ethcnn_pacer_policies_create(ethcnn_ctx* c, int nslots, const ethcnn_pacer_policy* policies, int npolicies, const int* slot_policy,
                                                ethcnn_pacer_set** out) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set_create: null output");
    if (nslots < 1 || nslots > kPacerSetMax) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set_create: %d slots (1..%d)", nslots, kPacerSetMax);
    if (int rc = check_policies(c, policies, npolicies, slot_policy, nslots)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // every ladder with its full search appended, one after another; a record per policy
    std::vector<int> rows;
    ethcnn_pacer_set* p = new ethcnn_pacer_set;
    p->c = c;
    p->nslots = nslots;
    p->npolicies = npolicies;
    for (int i = 0; i < npolicies; ++i) {
        const ethcnn_pacer_policy& q = policies[i];
        const std::vector<int> mine = ladder_rows(q.ladder, q.K);
        PolicyRec& r = p->policy[i];
        r.first_row = (int)(rows.size() / 6);
        r.rungs = (int)(mine.size() / 6);
        r.carry_mode = q.mode == ETHCNN_BUDGET_CARRY;
        r.budget_ppm = q.budget_ppm;
        for (int d = 0; d < 4; ++d) r.weight[d] = (q.weight ? q.weight : sim::kDefaultWeight)[d];
        rows.insert(rows.end(), mine.begin(), mine.end());
        p->stride = r.rungs > p->stride ? r.rungs : p->stride;
    }
    for (int s = 0; s < nslots; ++s) p->slot_policy[s] = slot_policy ? slot_policy[s] : 0;
    const size_t n = rows.size() / 6, recs = (size_t)npolicies * sizeof(PolicyRec), tables = (size_t)nslots * p->stride * 16,
                 states = (size_t)nslots * kStateWords * 4;
    hipError_t e = hipMalloc((void**)&p->d_thr, n * 24);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_policy, recs);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_checked, tables);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_state, states);
    if (e == hipSuccess) e = hipHostMalloc((void**)&p->h_result, (size_t)nslots * sizeof(ethcnn_pacer_result), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_thr, rows.data(), n * 24, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_policy, p->policy, recs, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_checked, 0, tables, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_state, 0, states, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (rows is a temporary)
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ethcnn_pacer_set_destroy(p);
        return set_err(c, e == hipErrorOutOfMemory ? ETHCNN_ERR_NOMEM : ETHCNN_ERR_DEVICE, "ethcnn_pacer_set_create: %s (%llu bytes of tables)", hipGetErrorString(e),
                       (unsigned long long)(n * 24 + recs + tables + states));
    }
    std::memset(p->h_result, 0, (size_t)nslots * sizeof *p->h_result);
    *out = p;
    return ETHCNN_OK;
}

extern "C" int ethcnn_pacer_set_create(ethcnn_ctx* c, int nslots, const ethcnn_sim_thr* ladder, int64_t K, const uint64_t weight[4], uint32_t budget_ppm,
                                       int mode, ethcnn_pacer_set** out) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set_create: null output");
    if (nslots < 1 || nslots > kPacerSetMax) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set_create: %d slots (1..%d)", nslots, kPacerSetMax);
    if (int rc = check_rules(c, ladder, K, weight, budget_ppm, mode)) return rc;  // (its messages without a policy index, as before)
    const ethcnn_pacer_policy one = {ladder, K, weight, budget_ppm, mode};
    return ethcnn_pacer_policies_create(c, nslots, &one, 1, nullptr, out);
}

extern "C" void ethcnn_pacer_set_destroy(ethcnn_pacer_set* p) {
    if (!p) return;
    if (p->c && p->c->stream) (void)hipStreamSynchronize(p->c->stream);
    if (p->d_thr) (void)hipFree(p->d_thr);
    if (p->d_policy) (void)hipFree(p->d_policy);
    if (p->d_checked) (void)hipFree(p->d_checked);
    if (p->d_state) (void)hipFree(p->d_state);
    if (p->d_recs) (void)hipFree(p->d_recs);
    if (p->d_stage) (void)hipFree(p->d_stage);
    if (p->h_result) (void)hipHostFree(p->h_result);
    delete p;
}

extern "C" int ethcnn_pacer_set_slots(const ethcnn_pacer_set* p) { return p ? p->nslots : ETHCNN_ERR_ARG; }

extern "C" int64_t ethcnn_pacer_set_launches(const ethcnn_pacer_set* p) { return p ? p->launches : ETHCNN_ERR_ARG; }

extern "C" int ethcnn_pacer_policies_count(const ethcnn_pacer_set* p) { return p ? p->npolicies : ETHCNN_ERR_ARG; }

extern "C" int ethcnn_pacer_policies_of(const ethcnn_pacer_set* p, int slot) {
    if (!p) return ETHCNN_ERR_ARG;
    if (slot < 0 || slot >= p->nslots) return set_err(p->c, ETHCNN_ERR_ARG, "ethcnn_pacer_policies_of: slot %d is outside 0..%d", slot, p->nslots - 1);
    return p->slot_policy[slot];
}

// carry = 0, frame = 0 and an all-zero table of one slot, in stream order behind the frames already queued
static int reset_slot(ethcnn_pacer_set* p, int slot) {
    ethcnn_ctx* c = p->c;
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;
    // (the slot's table and ticket are zero between calls anyway; the whole stride, whatever policy the slot had)
    HIPCHK(c, hipMemsetAsync(p->d_state + (size_t)slot * kStateWords, 0, kStateWords * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(p->d_checked + (size_t)slot * p->stride * 4, 0, (size_t)p->stride * 16, c->stream));
    p->queued[slot] = 0;
    return ETHCNN_OK;
}

extern "C" int ethcnn_pacer_set_reset(ethcnn_pacer_set* p, int slot) {
    if (!p) return ETHCNN_ERR_ARG;
    if (slot < 0 || slot >= p->nslots) return set_err(p->c, ETHCNN_ERR_ARG, "ethcnn_pacer_set_reset: slot %d is outside 0..%d", slot, p->nslots - 1);
    return reset_slot(p, slot);
}

extern "C" int ethcnn_pacer_policies_bind(ethcnn_pacer_set* p, int slot, int policy) {
    if (!p) return ETHCNN_ERR_ARG;
    if (slot < 0 || slot >= p->nslots) return set_err(p->c, ETHCNN_ERR_ARG, "ethcnn_pacer_policies_bind: slot %d is outside 0..%d", slot, p->nslots - 1);
    if (policy < 0 || policy >= p->npolicies) return set_err(p->c, ETHCNN_ERR_ARG, "ethcnn_pacer_policies_bind: policy %d is outside 0..%d", policy, p->npolicies - 1);
    if (int rc = reset_slot(p, slot)) return rc;
    // the frames already queued carry the old policy in their kernel argument: the binding is the host's, from the next call on
    p->slot_policy[slot] = policy;
    return ETHCNN_OK;
}

extern "C" int ethcnn_pacer_set_frames_device(ethcnn_pacer_set* p, const ethcnn_pacer_set_frame* frames, int n) {
    if (!p) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = p->c;
    Checked k;
    if (int rc = check_call(p, frames, n, true, &k)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = grow(c, (void**)&p->d_recs, &p->cap_recs, k.total, 64, "record scratch")) return rc;
    return enqueue(p, frames, n, k);
}

extern "C" int ethcnn_pacer_set_frames(ethcnn_pacer_set* p, const ethcnn_pacer_set_frame* frames, int n) {
    if (!p) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = p->c;
    Checked k;
    if (int rc = check_call(p, frames, n, false, &k)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // a pointer inside an ethcnn_host_alloc buffer is read / written in place by the kernels; a frame with any other pointer gets a
    // piece of the one staging buffer, which then holds its input, its output or both (in place)
    bool in_direct[kPacerSetMax], out_direct[kPacerSetMax];
    int64_t stage_at[kPacerSetMax], staged = 0;
    bool all_out_direct = true;
    for (int j = 0; j < n; ++j) {
        const size_t bytes = (size_t)k.per[j] * kNout * 4;
        in_direct[j] = in_pinned(c, frames[j].probs, bytes), out_direct[j] = in_pinned(c, frames[j].baked, bytes);
        stage_at[j] = staged;
        if (!in_direct[j] || !out_direct[j]) staged += k.per[j];
        all_out_direct = all_out_direct && out_direct[j];
    }
    if (int rc = grow(c, (void**)&p->d_recs, &p->cap_recs, k.total, 64, "record scratch")) return rc;
    if (int rc = grow(c, (void**)&p->d_stage, &p->cap_stage, staged, kNout * 4, "staging")) return rc;
    c->done_armed = 0;
    ethcnn_pacer_set_frame dev[kPacerSetMax];
    for (int j = 0; j < n; ++j) {
        float* stage = p->d_stage + stage_at[j] * kNout;
        dev[j] = frames[j];
        dev[j].result = nullptr;
        if (!in_direct[j]) {
            HIPCHK(c, hipMemcpyAsync(stage, frames[j].probs, (size_t)k.per[j] * kNout * 4, hipMemcpyHostToDevice, c->stream));
            dev[j].probs = stage;
        }
        if (!out_direct[j]) dev[j].baked = stage;
    }
    if (int rc = enqueue(p, dev, n, k)) return rc;
    for (int j = 0; j < n; ++j)
        if (!out_direct[j]) HIPCHK(c, hipMemcpyAsync(frames[j].baked, dev[j].baked, (size_t)k.per[j] * kNout * 4, hipMemcpyDeviceToHost, c->stream));
    if (!all_out_direct) HIPCHK(c, hipStreamSynchronize(c->stream));
    else {
        // the wait: a bounded spin on the completion word that one lane stores behind the bake, hipStreamSynchronize as the fallback
        const unsigned seq = done_arm(c);
        if (seq) {
            launch_done(c->stream, c->h_done, seq);
            HIPCHK(c, hipGetLastError());
            ++p->launches;
            c->done_armed = seq;
        }
        HIPCHK(c, stream_sync(c));
    }
    for (int j = 0; j < n; ++j)
        if (frames[j].result) *frames[j].result = p->h_result[frames[j].slot];
    return ETHCNN_OK;
}

extern "C" int ethcnn_pacer_set_last(ethcnn_pacer_set* p, int slot, ethcnn_pacer_result* out) {
    if (!p) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = p->c;
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set_last: null output");
    if (slot < 0 || slot >= p->nslots) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set_last: slot %d is outside 0..%d", slot, p->nslots - 1);
    if (p->queued[slot] == 0) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_pacer_set_last: slot %d has paced no frame since create / reset", slot);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_sync(c));
    *out = p->h_result[slot];
    return ETHCNN_OK;
}
