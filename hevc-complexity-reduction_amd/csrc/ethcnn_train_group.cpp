// ethcnn_train_group.cpp -- the step engine of ETH-CNN training and the trainer group's entry points (include/ethcnn.h "training,
// several models at once").  The engine is K >= 1 trainers of ethcnn_train.cpp that share a context, a stream, the two sample sets
// and every launch of a step (kernels and grid mapping: ethcnn_train.h "the member table").  A trainer group is an engine over its
// K members; a solo trainer's entry points (ethcnn_train.cpp) call the ones below on an engine over the trainer itself, so there is
// one step, one evaluation and one sample upload.  What is not a step (weights in and out, the QP list, the debug buffers) is the
// member's own business and goes through its trainer entry points.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ethcnn_ctx.h"
#include "ethcnn_samples.h"
#include "ethcnn_train.h"
#include "ethcnn_train_host.h"

using namespace ethcnn::train;
using ethcnn::kBlobFloats;

// a member's own entry point failed: its message, with the member named
static int from_member(ethcnn_train_group* g, int i, int rc) {
    if (rc) g->err = "member " + std::to_string(i) + ": " + g->m[(size_t)i]->err;
    return rc;
}
static int member_index(ethcnn_train_group* g, int i) {
    if (i < 0 || i >= g->K) return terr(g, ETHCNN_ERR_ARG, "member %d outside 0..%d", i, g->K - 1);
    return 0;
}
static const char* api(const ethcnn_train_group* g) { return g->group ? "ethcnn_train_group" : "ethcnn_train"; }

extern "C" int ethcnn_train_group_check(const ethcnn_train_options* opts, int k, char* err, size_t errcap) {
    char buf[256] = "";
    int rc = ETHCNN_OK;
    const auto fail = [&](const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        rc = ETHCNN_ERR_ARG;
    };
    if (k < 1 || k > kMaxMembers) fail("a trainer group holds 1..%d members, got k = %d", kMaxMembers, k);
    else if (!opts) fail("no options");
    for (int i = 0; rc == ETHCNN_OK && i < k; ++i) {
        const ethcnn_train_options& o = opts[i];
        if (o.batch <= 0 || o.batch > 65536) fail("member %d: batch must be in 1..65536, got %d", i, o.batch);
        else if (o.decay_steps <= 0) fail("member %d: decay_steps must be positive", i);
        else if (!std::isfinite(o.lr_init)) fail("member %d: lr_init is not finite", i);
        else if (!std::isfinite(o.momentum)) fail("member %d: momentum is not finite", i);
        else if (!std::isfinite(o.decay_rate)) fail("member %d: decay_rate is not finite", i);
        else if (o.net != ETHCNN_TRAIN_NET_AI && o.net != ETHCNN_TRAIN_NET_LDP)
            fail("member %d: net must be %d (All-Intra) or %d (LDP), got %d", i, ETHCNN_TRAIN_NET_AI, ETHCNN_TRAIN_NET_LDP, o.net);
        else if (o.tune < 0 || o.tune > 3) fail("member %d: tune must be in 0..3, got %d", i, o.tune);
        else if (o.net != opts[0].net) fail("member %d: net %d differs from member 0's %d (one net per group)", i, o.net, opts[0].net);
        else if (o.batch != opts[0].batch)
            fail("member %d: batch %d differs from member 0's %d (one batch size per group)", i, o.batch, opts[0].batch);
        else if (o.tune != opts[0].tune) fail("member %d: tune %d differs from member 0's %d (one tuning mode per group)", i, o.tune, opts[0].tune);
    }
    if (err && errcap) std::snprintf(err, errcap, "%s", buf);
    return rc;
}

// the table of a training step, from the members as they are now
static Member member_entry(const ethcnn_trainer* t) {
    Member e{};
    e.W = t->W; e.acc = t->acc; e.grad = t->grad;
    e.idx_in = t->idx_in; e.qp_in = t->qp_in; e.idx = t->idx; e.qp = t->qp;
    e.lab = t->lab; e.trunk = t->trunk; e.F = t->F; e.Z1 = t->Z1; e.A1 = t->A1; e.M1 = t->M1; e.H1 = t->H1; e.A2 = t->A2; e.M2 = t->M2;
    e.H2 = t->H2; e.P = t->P; e.dZ3 = t->dZ3; e.dZ2 = t->dZ2; e.dZ1 = t->dZ1; e.dF = t->dF; e.part = t->part; e.stats = t->stats;
    e.seed = t->opt.seed;
    std::memcpy(e.qps, t->qps, sizeof e.qps);
    e.nqps = t->nqps;
    e.qp_fixed = -1;
    e.dropout = t->opt.dropout ? 1 : 0;
    e.momentum = t->opt.momentum;
    return e;
}

static int upload_table(ethcnn_train_group* g) {
    if (!g->stale) return 0;
    std::vector<Member> tab;
    for (const ethcnn_trainer* t : g->m) tab.push_back(member_entry(t));
    TCHK(g, hipStreamSynchronize(g->c->stream));  // steps in flight still read the old table
    TCHK(g, hipMemcpy(g->d_tab, tab.data(), sizeof(Member) * tab.size(), hipMemcpyHostToDevice));
    g->stale = false;
    return 0;
}

static GroupStep step_args(const ethcnn_train_group* g, int set, uint64_t step, int drawn) {
    GroupStep s{};
    s.data = g->data[set];
    s.nrec = g->nrec[set];
    std::memcpy(s.slot_of_qp, g->slot_of_qp[set], sizeof s.slot_of_qp);
    s.step = step;
    s.drawn = drawn;
    return s;
}

static int enqueue_step(ethcnn_train_group* g, int64_t step, bool explicit_batch) {
    hipStream_t s = g->c->stream;
    const NetOffsets& o = g->m[0]->o;
    g->c->done_armed = 0;  // the context's completion word does not cover these launches
    GroupRates r{};
    for (int i = 0; i < g->K; ++i) {
        const ethcnn_train_options& p = g->m[(size_t)i]->opt;
        r.lr[i] = lr_at(p.lr_init, p.decay_rate, p.decay_steps, step);
    }
    launch_group_trunk_fwd(s, g->B, g->K, g->d_tab, step_args(g, ETHCNN_TRAIN_SET_TRAIN, (uint64_t)step, explicit_batch ? 0 : 1), o, g->net);
    launch_group_gemm(s, g->d_fwd, g->t_fwd, g->K);
    launch_group_heads_fwd(s, g->B, g->K, g->d_tab, o, (uint64_t)step, g->net);
    launch_group_loss(s, g->K, g->d_tab, g->B, 1);
    launch_group_heads_bwd(s, g->B, g->K, g->d_tab, o);
    launch_group_gemm(s, g->d_bwd, g->t_bwd, g->K);
    if (!g->tune) launch_group_trunk_bwd(s, g->B, g->K, g->d_tab, o);
    launch_group_update(s, g->K, g->d_tab, g->B, r, (long)kBlobFloats, g->m[0]->mask);
    TCHK(g, hipGetLastError());
    return 0;
}

static int read_stats(ethcnn_train_group* g, float* loss, float* acc) {
    float* st[kMaxMembers];
    for (int i = 0; i < g->K; ++i) st[i] = g->m[(size_t)i]->stats;
    TCHK(g, ethcnn::train::read_stats(g->c->stream, st, g->K, loss, acc));
    return 0;
}

static int ready(ethcnn_train_group* g) {
    if (!g->data[ETHCNN_TRAIN_SET_TRAIN]) return terr(g, ETHCNN_ERR_ARG, "no training samples (%s_set_samples)", api(g));
    for (int i = 0; i < g->K; ++i)
        if (!g->m[(size_t)i]->nqps) return gerr(g, i, ETHCNN_ERR_ARG, "no QP list (%s_set_qps)", api(g));
    return 0;
}

void train_engine_destroy(ethcnn_train_group* g) {
    if (!g) return;
    for (int s = 0; s < 2; ++s) (void)hipFree(g->data[s]);
    (void)hipFree(g->d_tab);
    (void)hipFree(g->d_fwd);
    (void)hipFree(g->d_bwd);
    (void)hipFree(g->d_eval);
    delete g;
}

int train_engine_create(ethcnn_ctx* c, const std::vector<ethcnn_trainer*>& members, bool group, ethcnn_train_group** out) {
    ethcnn_train_group* g = new (std::nothrow) ethcnn_train_group;
    if (!g) return set_err(c, ETHCNN_ERR_NOMEM, "out of memory");
    const ethcnn_trainer* t0 = members[0];
    g->c = c;
    g->m = members;
    g->K = (int)members.size();
    g->B = t0->B;
    g->cap = t0->cap;
    g->net = t0->net;
    g->tune = t0->tune;
    g->group = group;
    for (int s = 0; s < 2; ++s)
        for (int q = 0; q < 52; ++q) g->slot_of_qp[s][q] = -1;
    std::vector<GemmGroup> gf, gb, ge;
    for (const ethcnn_trainer* t : g->m) {
        gf.push_back(train_fc1_group(t, g->B));
        gb.push_back(train_bwd_group(t, g->B));
        ge.push_back(train_fc1_group(t, g->cap));
    }
    g->t_fwd = gf[0].tiles; g->t_bwd = gb[0].tiles; g->t_eval = ge[0].tiles;
    const size_t gbytes = sizeof(GemmGroup) * (size_t)g->K;
    hipError_t e = hipMalloc((void**)&g->d_tab, sizeof(Member) * (size_t)g->K);
    e = e ? e : hipMalloc((void**)&g->d_fwd, gbytes);
    e = e ? e : hipMalloc((void**)&g->d_bwd, gbytes);
    e = e ? e : hipMalloc((void**)&g->d_eval, gbytes);
    e = e ? e : hipMemcpy(g->d_fwd, gf.data(), gbytes, hipMemcpyHostToDevice);
    e = e ? e : hipMemcpy(g->d_bwd, gb.data(), gbytes, hipMemcpyHostToDevice);
    e = e ? e : hipMemcpy(g->d_eval, ge.data(), gbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        train_engine_destroy(g);
        return set_err(c, ETHCNN_ERR_DEVICE, "%s setup: %s", group ? "trainer group" : "trainer", hipGetErrorString(e));
    }
    for (ethcnn_trainer* t : g->m) t->eng = g;
    *out = g;
    return ETHCNN_OK;
}

extern "C" void ethcnn_train_group_destroy(ethcnn_train_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->c->device);
    (void)hipStreamSynchronize(g->c->stream);
    for (ethcnn_trainer* t : g->m) train_member_destroy(t);
    train_engine_destroy(g);
}

extern "C" int ethcnn_train_group_create(ethcnn_ctx* c, const ethcnn_train_options* opts, int k, ethcnn_train_group** out) {
    if (!c || !out) return ETHCNN_ERR_ARG;
    *out = nullptr;
    char why[256];
    if (int rc = ethcnn_train_group_check(opts, k, why, sizeof why)) return set_err(c, rc, "%s", why);
    std::vector<ethcnn_trainer*> m;
    int rc = 0;
    for (int i = 0; i < k && !rc; ++i) {
        ethcnn_trainer* t = nullptr;
        rc = train_member_create(c, &opts[i], &t);  // (the context holds the message)
        if (!rc) m.push_back(t);
    }
    rc = rc ? rc : train_engine_create(c, m, true, out);
    if (rc)
        for (ethcnn_trainer* t : m) train_member_destroy(t);
    return rc;
}

extern "C" const char* ethcnn_train_group_last_error(const ethcnn_train_group* g) { return g ? g->err.c_str() : "trainer group is NULL"; }

extern "C" int ethcnn_train_group_init_weights(ethcnn_train_group* g, const uint64_t* seeds) {
    if (!g) return ETHCNN_ERR_ARG;
    if (!seeds) return terr(g, ETHCNN_ERR_ARG, "no seeds");
    for (int i = 0; i < g->K; ++i)
        if (int rc = from_member(g, i, ethcnn_train_init_weights(g->m[(size_t)i], seeds[i]))) return rc;
    return 0;
}

extern "C" int ethcnn_train_group_set_blob(ethcnn_train_group* g, int i, const float* blob, const float* accum, size_t n) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = member_index(g, i)) return rc;
    return from_member(g, i, ethcnn_train_set_blob(g->m[(size_t)i], blob, accum, n));
}

extern "C" int ethcnn_train_group_get_blob(ethcnn_train_group* g, int i, float* blob, float* accum, size_t n) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = member_index(g, i)) return rc;
    return from_member(g, i, ethcnn_train_get_blob(g->m[(size_t)i], blob, accum, n));
}

static void drop_set(ethcnn_train_group* g, int set) {
    (void)hipFree(g->data[set]);
    g->data[set] = nullptr;
    g->nrec[set] = 0;
    g->stale = true;
}

// the checks every record takes on the device, then the set's bookkeeping: `p` (n records in HBM) becomes set `set`.  LDP: every record
// carries the slot QPs sq[4] (one pass on the device).  On failure `p` is left to the caller.
static int install_samples(ethcnn_train_group* g, int set, uint8_t* p, int64_t n, const int sq[4]) {
    if (g->net == kNetLdp) {
        const int nblk = (int)std::min<int64_t>(1024, (n + 255) / 256);
        long* d_bad = nullptr;
        std::vector<long> bad((size_t)nblk);
        const uint32_t want = (uint32_t)sq[0] | (uint32_t)sq[1] << 8 | (uint32_t)sq[2] << 16 | (uint32_t)sq[3] << 24;
        hipError_t e = hipMalloc(&d_bad, sizeof(long) * nblk);
        if (e == hipSuccess) {
            launch_check_slots(g->c->stream, p, (long)n, want, d_bad, nblk);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(bad.data(), d_bad, sizeof(long) * nblk, hipMemcpyDeviceToHost, g->c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g->c->stream);
        (void)hipFree(d_bad);
        if (e != hipSuccess) return terr(g, ETHCNN_ERR_DEVICE, "sample check: %s", hipGetErrorString(e));
        const long first = *std::min_element(bad.begin(), bad.end());
        if (first < n) {
            uint8_t r[3 * kSlotBytes + 1] = {0};
            (void)hipMemcpy(r, p + (size_t)first * kRecLdp + kSlotBase, sizeof r, hipMemcpyDeviceToHost);
            return terr(g, ETHCNN_ERR_FORMAT, "record %ld: slot QPs %d %d %d %d differ from record 0's %d %d %d %d", first, r[0],
                        r[kSlotBytes], r[2 * kSlotBytes], r[3 * kSlotBytes], sq[0], sq[1], sq[2], sq[3]);
        }
    }
    drop_set(g, set);
    if (g->net == kNetLdp) {
        for (int q = 0; q < 52; ++q) g->slot_of_qp[set][q] = -1;
        for (int q = 0; q < 4; ++q) {
            g->slot_qps[set][q] = sq[q];
            g->slot_of_qp[set][sq[q]] = q;
        }
        if (set == ETHCNN_TRAIN_SET_TRAIN)  // every member's QP list defaults to the four slots (every MODEL_TYPE trains on all of them)
            for (ethcnn_trainer* t : g->m) {
                std::memcpy(t->qps, sq, sizeof(int) * 4);
                t->nqps = 4;
            }
    }
    g->data[set] = p;
    g->nrec[set] = n;
    return 0;
}

extern "C" int ethcnn_train_group_set_samples(ethcnn_train_group* g, int set, const uint8_t* rec, size_t nbytes) {
    if (!g) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return terr(g, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    if (!rec || nbytes == 0) return terr(g, ETHCNN_ERR_ARG, "no sample records");
    const int rb = g->net == kNetLdp ? kRecLdp : kRec;
    if (nbytes % rb) return terr(g, ETHCNN_ERR_FORMAT, "%zu bytes is not a whole number of %d-byte records", nbytes, rb);
    if (nbytes / rb > 0x7fffffffull) return terr(g, ETHCNN_ERR_ARG, "more than 2^31 - 1 records");
    int sq[4] = {0, 0, 0, 0};
    if (g->net == kNetLdp) {  // record 0's slot QPs: four distinct values in 0..51
        for (int q = 0; q < 4; ++q) {
            sq[q] = rec[kSlotBase + kSlotBytes * q];
            if (sq[q] > 51) return terr(g, ETHCNN_ERR_FORMAT, "record 0: slot %d holds QP %d, outside 0..51", q, sq[q]);
            for (int k = 0; k < q; ++k)
                if (sq[k] == sq[q]) return terr(g, ETHCNN_ERR_FORMAT, "record 0: slots %d and %d both hold QP %d", k, q, sq[q]);
        }
    }
    TCHK(g, hipSetDevice(g->c->device));
    TCHK(g, hipStreamSynchronize(g->c->stream));
    drop_set(g, set);  // before the new copy is allocated: the two need not fit side by side
    void* p = nullptr;
    if (hipMalloc(&p, nbytes) != hipSuccess) {
        (void)hipGetLastError();
        return terr(g, ETHCNN_ERR_NOMEM, "%zu bytes of samples do not fit in device memory", nbytes);
    }
    if (hipMemcpy(p, rec, nbytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p);
        return terr(g, ETHCNN_ERR_DEVICE, "sample upload failed");
    }
    const int rc = install_samples(g, set, (uint8_t*)p, (int64_t)(nbytes / rb), sq);
    if (rc) (void)hipFree(p);
    return rc;
}

// the same from a sample set already in HBM (include/ethcnn.h "sample sets"): adopted (take) or copied device to device
extern "C" int ethcnn_train_group_set_samples_from(ethcnn_train_group* g, int set, ethcnn_samples* sm, int take) {
    if (!g) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return terr(g, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    if (!sm || !sm->built || sm->count == 0) return terr(g, ETHCNN_ERR_ARG, "no sample records (the sample set is not built or empty)");
    if (sm->c != g->c) return terr(g, ETHCNN_ERR_ARG, "the sample set and the trainer live on different contexts");
    if (sm->kind != g->net)
        return terr(g, ETHCNN_ERR_FORMAT, "a sample set of %d-byte records does not feed this trainer's net (%d-byte records)",
                    sm->record_bytes(), g->net == kNetLdp ? kRecLdp : kRec);
    if (sm->count > 0x7fffffffll) return terr(g, ETHCNN_ERR_ARG, "more than 2^31 - 1 records");
    TCHK(g, hipSetDevice(g->c->device));
    TCHK(g, hipStreamSynchronize(g->c->stream));
    const size_t nbytes = (size_t)sm->count * (size_t)sm->record_bytes();
    uint8_t* p = sm->data;
    if (!take) {
        if (hipMalloc((void**)&p, nbytes) != hipSuccess) {
            (void)hipGetLastError();
            return terr(g, ETHCNN_ERR_NOMEM, "%zu bytes of samples do not fit in device memory", nbytes);
        }
        // (on the context's stream, which does not wait for the null stream: a device-to-device hipMemcpy there may still be
        // running when the check below reads its destination)
        if (hipMemcpyAsync(p, sm->data, nbytes, hipMemcpyDeviceToDevice, g->c->stream) != hipSuccess ||
            hipStreamSynchronize(g->c->stream) != hipSuccess) {
            (void)hipFree(p);
            return terr(g, ETHCNN_ERR_DEVICE, "sample copy failed");
        }
    }
    const int rc = install_samples(g, set, p, sm->count, sm->qps);
    if (rc) {
        if (!take) (void)hipFree(p);
        return rc;
    }
    if (take) {  // the engine owns the buffer now; the set is empty (and may take sequences again)
        sm->data = nullptr;
        sm->count = 0;
        sm->seqs.clear();
        sm->built = false;
    }
    return 0;
}

extern "C" int ethcnn_train_group_set_qps(ethcnn_train_group* g, int i, const int* qps, int n) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = member_index(g, i)) return rc;
    return from_member(g, i, ethcnn_train_set_qps(g->m[(size_t)i], qps, n));  // (marks the table stale)
}

extern "C" int ethcnn_train_group_run(ethcnn_train_group* g, int64_t first_step, int64_t nsteps) {
    if (!g) return ETHCNN_ERR_ARG;
    if (first_step < 0 || nsteps < 0) return terr(g, ETHCNN_ERR_ARG, "negative step");
    if (int rc = ready(g)) return rc;
    TCHK(g, hipSetDevice(g->c->device));
    if (int rc = upload_table(g)) return rc;
    for (int64_t i = 0; i < nsteps; ++i)
        if (int rc = enqueue_step(g, first_step + i, false)) return rc;
    return 0;
}

extern "C" int ethcnn_train_group_last_stats(ethcnn_train_group* g, float* loss, float* acc) {
    if (!g) return ETHCNN_ERR_ARG;
    TCHK(g, hipSetDevice(g->c->device));
    return read_stats(g, loss, acc);
}

extern "C" int ethcnn_train_group_step_indices(ethcnn_train_group* g, int64_t step, const int32_t* idx, const int* qp, int n, float* loss,
                                               float* acc) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = ready(g)) return rc;
    if (!idx || !qp || n != g->B)
        return terr(g, ETHCNN_ERR_ARG, "an explicit batch needs %d indices and QPs%s", g->B, g->group ? " per member" : "");
    if (step < 0) return terr(g, ETHCNN_ERR_ARG, "negative step");
    for (int i = 0; i < g->K * n; ++i) {
        if (idx[i] < 0 || idx[i] >= g->nrec[0])
            return gerr(g, i / n, ETHCNN_ERR_ARG, "sample index %d outside 0..%lld", idx[i], (long long)g->nrec[0] - 1);
        if (qp[i] < 0 || qp[i] > 51) return gerr(g, i / n, ETHCNN_ERR_ARG, "QP %d outside 0..51", qp[i]);
        if (g->net == kNetLdp && g->slot_of_qp[ETHCNN_TRAIN_SET_TRAIN][qp[i]] < 0)
            return gerr(g, i / n, ETHCNN_ERR_ARG, "QP %d is not a slot QP of the training samples", qp[i]);
    }
    TCHK(g, hipSetDevice(g->c->device));
    if (int rc = upload_table(g)) return rc;
    hipStream_t s = g->c->stream;
    for (int i = 0; i < g->K; ++i) {
        TCHK(g, hipMemcpyAsync(g->m[(size_t)i]->idx_in, idx + (size_t)i * n, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
        TCHK(g, hipMemcpyAsync(g->m[(size_t)i]->qp_in, qp + (size_t)i * n, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    }
    TCHK(g, hipStreamSynchronize(s));
    if (int rc = enqueue_step(g, step, true)) return rc;
    return read_stats(g, loss, acc);
}

extern "C" int ethcnn_train_group_evaluate(ethcnn_train_group* g, int set, const int32_t* idx, int64_t n, const int* qps, float* loss,
                                           float* acc, float* probs) {
    if (!g) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return terr(g, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    if (!g->data[set]) return terr(g, ETHCNN_ERR_ARG, "no samples in set %d", set);
    if (!qps) return terr(g, ETHCNN_ERR_ARG, "no QPs");
    const bool ldp = g->net == kNetLdp;
    const int K = g->K;
    bool any_mixed = false;
    for (int i = 0; i < K; ++i) {
        const int qp = qps[i];
        if (!(qp >= 0 && qp <= 51) && !(ldp && qp == -1))
            return gerr(g, i, ETHCNN_ERR_ARG, ldp ? "QP %d is neither a slot QP nor -1" : "QP %d outside 0..51", qp);
        if (ldp && qp >= 0 && g->slot_of_qp[set][qp] < 0) return gerr(g, i, ETHCNN_ERR_ARG, "QP %d is not a slot QP of set %d", qp, set);
        any_mixed = any_mixed || qp < 0;
    }
    if (n <= 0 || n > 0x7fffffffll || (!idx && n > g->nrec[set])) return terr(g, ETHCNN_ERR_ARG, "bad sample count %lld", (long long)n);
    if (idx)
        for (int64_t i = 0; i < n; ++i)
            if (idx[i] < 0 || idx[i] >= g->nrec[set])
                return terr(g, ETHCNN_ERR_ARG, "sample index %d outside 0..%lld", idx[i], (long long)g->nrec[set] - 1);
    TCHK(g, hipSetDevice(g->c->device));
    hipStream_t s = g->c->stream;
    g->c->done_armed = 0;
    std::vector<int32_t> ids;
    if (!idx) {
        ids.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) ids[(size_t)i] = (int32_t)i;
        idx = ids.data();
    }
    // qp == -1: member m's sample i at the slot its own draw(2, 0, i, 0) picks among the four
    std::vector<int32_t> mixed;
    if (any_mixed) {
        mixed.assign((size_t)K * (size_t)n, 0);
        for (int m = 0; m < K; ++m)
            if (qps[m] < 0)
                for (int64_t i = 0; i < n; ++i)
                    mixed[(size_t)m * n + i] = g->slot_qps[set][((draw(g->m[(size_t)m]->opt.seed, kStreamQp, 0, (uint64_t)i, 0) >> 32) * 4ull) >> 32];
    }
    // one table per piece (launches 1-3) and one for the loss launch over all n; the tables and the indices share ONE allocation and
    // ONE upload, staged in `host`: [tables | indices]
    const int64_t pieces = (n + g->cap - 1) / g->cap;
    const size_t tab_bytes = sizeof(Member) * (size_t)K * (size_t)(pieces + 1), in_bytes = (size_t)n * 4;
    float *Pn = nullptr, *Ln = nullptr;
    int32_t* Qn = nullptr;
    uint8_t* D = nullptr;
    const auto release = [&]() { (void)hipFree(Pn); (void)hipFree(Ln); (void)hipFree(Qn); (void)hipFree(D); };
    if (hipMalloc((void**)&Pn, (size_t)K * n * kTOut * 4) != hipSuccess || hipMalloc((void**)&Ln, (size_t)K * n * 16 * 4) != hipSuccess ||
        hipMalloc((void**)&D, tab_bytes + in_bytes) != hipSuccess || (any_mixed && hipMalloc((void**)&Qn, (size_t)K * n * 4) != hipSuccess)) {
        (void)hipGetLastError();
        release();
        return terr(g, ETHCNN_ERR_NOMEM, "cannot allocate the evaluation buffers of %d x %lld samples", K, (long long)n);
    }
    Member* d_tabs = (Member*)D;
    int32_t* In = (int32_t*)(D + tab_bytes);
    std::vector<uint8_t> host(tab_bytes + in_bytes);
    Member* tabs = (Member*)host.data();
    std::memcpy(host.data() + tab_bytes, idx, in_bytes);
    for (int64_t p = 0; p <= pieces; ++p) {
        const int64_t c0 = p < pieces ? p * g->cap : 0;  // the last table: the loss launch, every member's whole P and labels
        for (int m = 0; m < K; ++m) {
            Member e = member_entry(g->m[(size_t)m]);
            e.idx_in = In + c0;
            e.qp_in = qps[m] < 0 ? Qn + (size_t)m * n + c0 : nullptr;
            e.qp_fixed = qps[m];
            e.dropout = 0;
            e.P = Pn + ((size_t)m * n + c0) * kTOut;
            e.lab = Ln + ((size_t)m * n + c0) * 16;
            tabs[p * K + m] = e;
        }
    }
    hipError_t e = hipMemcpyAsync(D, host.data(), host.size(), hipMemcpyHostToDevice, s);  // (`host` lives until the last synchronisation)
    if (e == hipSuccess && Qn) e = hipMemcpyAsync(Qn, mixed.data(), mixed.size() * 4, hipMemcpyHostToDevice, s);
    const NetOffsets& o = g->m[0]->o;
    for (int64_t p = 0; e == hipSuccess && p < pieces; ++p) {
        const int nb = (int)std::min<int64_t>(g->cap, n - p * g->cap);
        const Member* tab = d_tabs + p * K;
        launch_group_trunk_fwd(s, nb, K, tab, step_args(g, set, 0, 0), o, g->net);
        launch_group_gemm(s, g->d_eval, g->t_eval, K);
        launch_group_heads_fwd(s, nb, K, tab, o, 0, g->net);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        launch_group_loss(s, K, d_tabs + pieces * K, (int)n, 0);  // per member ONE batch over all n samples
        e = hipGetLastError();
    }
    if (e == hipSuccess && probs) e = hipMemcpyAsync(probs, Pn, (size_t)K * n * kTOut * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    release();
    if (e != hipSuccess) return terr(g, ETHCNN_ERR_DEVICE, "evaluation: %s", hipGetErrorString(e));
    return read_stats(g, loss, acc);
}

extern "C" int ethcnn_train_group_debug_fetch(ethcnn_train_group* g, int i, int which, float* out, size_t nfloats) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = member_index(g, i)) return rc;
    return from_member(g, i, ethcnn_train_debug_fetch(g->m[(size_t)i], which, out, nfloats));
}
