// ethcnn_train_group.cpp -- host side of the trainer group (include/ethcnn.h "training, several models at once"): K trainers of
// ethcnn_train.cpp that share a context, a stream, the two sample sets and every launch of a step (kernels and grid mapping:
// ethcnn_train.h "trainer group").  A member IS a solo trainer object: its buffers, weights, QP list and options are the solo ones,
// so everything that is not a step (weights in and out, the QP list, the debug buffers) goes through the solo entry points.
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

namespace ethcnn {
namespace train {
void launch_group_trunk_fwd(hipStream_t s, int nb, int k, const Member* tab, const GroupStep& g, const NetOffsets& o, int net);
void launch_group_gemm(hipStream_t s, const GemmGroup* d_grps, int tiles_per, int k);
void launch_group_heads_fwd(hipStream_t s, int nb, int k, const Member* tab, const NetOffsets& o, uint64_t step, int net);
void launch_group_loss(hipStream_t s, int k, const Member* tab, int n, int with_grad);
void launch_group_heads_bwd(hipStream_t s, int nb, int k, const Member* tab, const NetOffsets& o);
void launch_group_trunk_bwd(hipStream_t s, int nb, int k, const Member* tab, const NetOffsets& o);
void launch_group_update(hipStream_t s, int k, const Member* tab, int nb, const GroupRates& r, long n, const TuneMask& mask);
}  // namespace train
}  // namespace ethcnn

using namespace ethcnn::train;
using ethcnn::kBlobFloats;

struct ethcnn_train_group {
    ethcnn_ctx* c = nullptr;
    int K = 0, B = 0, cap = 0, net = kNetAi, tune = 0;
    std::vector<ethcnn_trainer*> m;  // member 0 owns the sample sets; the others hold the same pointers (cleared before destroy)
    Member* d_tab = nullptr;         // the member table of a training step
    GemmGroup *d_fwd = nullptr, *d_bwd = nullptr, *d_eval = nullptr;  // [K] each, side by side
    int t_fwd = 0, t_bwd = 0, t_eval = 0;                             // tiles of ONE member
    bool table_stale = true;  // a QP list changed since the table was uploaded
    std::string err;
};

static int gerr(ethcnn_train_group* g, int code, const char* fmt, ...) {
    char buf[640];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g->err = buf;
    return code;
}
#define GCHK(g, call)                                                                                           \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess) return gerr((g), ETHCNN_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// a member's own entry point failed: its message, with the member named
static int from_member(ethcnn_train_group* g, int i, int rc) {
    if (rc) g->err = "member " + std::to_string(i) + ": " + g->m[(size_t)i]->err;
    return rc;
}
static int member_index(ethcnn_train_group* g, int i) {
    if (i < 0 || i >= g->K) return gerr(g, ETHCNN_ERR_ARG, "member %d outside 0..%d", i, g->K - 1);
    return 0;
}

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
    if (!g->table_stale) return 0;
    std::vector<Member> tab;
    for (const ethcnn_trainer* t : g->m) tab.push_back(member_entry(t));
    GCHK(g, hipStreamSynchronize(g->c->stream));  // steps in flight still read the old table
    GCHK(g, hipMemcpy(g->d_tab, tab.data(), sizeof(Member) * tab.size(), hipMemcpyHostToDevice));
    g->table_stale = false;
    return 0;
}

static GroupStep step_args(const ethcnn_train_group* g, int set, uint64_t step, int drawn) {
    const ethcnn_trainer* t0 = g->m[0];
    GroupStep s{};
    s.data = t0->data[set];
    s.nrec = t0->nrec[set];
    std::memcpy(s.slot_of_qp, t0->slot_of_qp[set], sizeof s.slot_of_qp);
    s.step = step;
    s.drawn = drawn;
    return s;
}

static int enqueue_step(ethcnn_train_group* g, int64_t step, bool explicit_batch) {
    hipStream_t s = g->c->stream;
    const NetOffsets& o = g->m[0]->o;
    g->c->done_armed = 0;  // the context's completion word does not cover these launches
    GroupRates r{};
    for (int i = 0; i < g->K; ++i) r.lr[i] = train_lr_at(g->m[(size_t)i], step);
    launch_group_trunk_fwd(s, g->B, g->K, g->d_tab, step_args(g, ETHCNN_TRAIN_SET_TRAIN, (uint64_t)step, explicit_batch ? 0 : 1), o, g->net);
    launch_group_gemm(s, g->d_fwd, g->t_fwd, g->K);
    launch_group_heads_fwd(s, g->B, g->K, g->d_tab, o, (uint64_t)step, g->net);
    launch_group_loss(s, g->K, g->d_tab, g->B, 1);
    launch_group_heads_bwd(s, g->B, g->K, g->d_tab, o);
    launch_group_gemm(s, g->d_bwd, g->t_bwd, g->K);
    if (!g->tune) launch_group_trunk_bwd(s, g->B, g->K, g->d_tab, o);
    launch_group_update(s, g->K, g->d_tab, g->B, r, (long)kBlobFloats, g->m[0]->mask);
    GCHK(g, hipGetLastError());
    return 0;
}

static int read_stats(ethcnn_train_group* g, float* loss, float* acc) {
    float st[kMaxMembers][8];
    for (int i = 0; i < g->K; ++i)
        GCHK(g, hipMemcpyAsync(st[i], g->m[(size_t)i]->stats, sizeof st[i], hipMemcpyDeviceToHost, g->c->stream));
    GCHK(g, hipStreamSynchronize(g->c->stream));
    for (int i = 0; i < g->K; ++i)
        for (int l = 0; l < 3; ++l) {
            if (loss) loss[3 * i + l] = st[i][l];
            if (acc) acc[3 * i + l] = st[i][3 + l];
        }
    return 0;
}

static int ready(ethcnn_train_group* g) {  // the solo trainer's conditions and codes
    if (!g->m[0]->data[ETHCNN_TRAIN_SET_TRAIN]) return gerr(g, ETHCNN_ERR_ARG, "no training samples (ethcnn_train_group_set_samples)");
    for (int i = 0; i < g->K; ++i)
        if (!g->m[(size_t)i]->nqps) return gerr(g, ETHCNN_ERR_ARG, "member %d: no QP list (ethcnn_train_group_set_qps)", i);
    return 0;
}

extern "C" void ethcnn_train_group_destroy(ethcnn_train_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->c->device);
    (void)hipStreamSynchronize(g->c->stream);
    for (size_t i = 0; i < g->m.size(); ++i) {
        if (i)  // the sets are member 0's to free
            for (int s = 0; s < 2; ++s) g->m[i]->data[s] = nullptr;
        ethcnn_train_destroy(g->m[i]);
    }
    (void)hipFree(g->d_tab);
    (void)hipFree(g->d_fwd);
    (void)hipFree(g->d_bwd);
    (void)hipFree(g->d_eval);
    delete g;
}

extern "C" int ethcnn_train_group_create(ethcnn_ctx* c, const ethcnn_train_options* opts, int k, ethcnn_train_group** out) {
    if (!c || !out) return ETHCNN_ERR_ARG;
    *out = nullptr;
    char why[256];
    if (int rc = ethcnn_train_group_check(opts, k, why, sizeof why)) return set_err(c, rc, "%s", why);
    ethcnn_train_group* g = new (std::nothrow) ethcnn_train_group;
    if (!g) return set_err(c, ETHCNN_ERR_NOMEM, "out of memory");
    g->c = c;
    g->K = k;
    g->B = opts[0].batch;
    g->net = opts[0].net;
    g->tune = opts[0].tune;
    for (int i = 0; i < k; ++i) {
        ethcnn_trainer* t = nullptr;
        if (int rc = ethcnn_train_create(c, &opts[i], &t)) {  // (the context holds the message)
            ethcnn_train_group_destroy(g);
            return rc;
        }
        g->m.push_back(t);
    }
    g->cap = g->m[0]->cap;
    std::vector<GemmGroup> gf, gb, ge;
    for (const ethcnn_trainer* t : g->m) {
        gf.push_back(train_fc1_group(t, g->B));
        gb.push_back(train_bwd_group(t, g->B));
        ge.push_back(train_fc1_group(t, g->cap));
    }
    g->t_fwd = gf[0].tiles; g->t_bwd = gb[0].tiles; g->t_eval = ge[0].tiles;
    const size_t gbytes = sizeof(GemmGroup) * (size_t)k;
    hipError_t e = hipMalloc((void**)&g->d_tab, sizeof(Member) * (size_t)k);
    e = e ? e : hipMalloc((void**)&g->d_fwd, gbytes);
    e = e ? e : hipMalloc((void**)&g->d_bwd, gbytes);
    e = e ? e : hipMalloc((void**)&g->d_eval, gbytes);
    e = e ? e : hipMemcpy(g->d_fwd, gf.data(), gbytes, hipMemcpyHostToDevice);
    e = e ? e : hipMemcpy(g->d_bwd, gb.data(), gbytes, hipMemcpyHostToDevice);
    e = e ? e : hipMemcpy(g->d_eval, ge.data(), gbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ethcnn_train_group_destroy(g);
        return set_err(c, ETHCNN_ERR_DEVICE, "trainer group setup: %s", hipGetErrorString(e));
    }
    *out = g;
    return ETHCNN_OK;
}

extern "C" const char* ethcnn_train_group_last_error(const ethcnn_train_group* g) { return g ? g->err.c_str() : "trainer group is NULL"; }

extern "C" int ethcnn_train_group_init_weights(ethcnn_train_group* g, const uint64_t* seeds) {
    if (!g) return ETHCNN_ERR_ARG;
    if (!seeds) return gerr(g, ETHCNN_ERR_ARG, "no seeds");
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

// member 0 took (or lost) a set through its solo entry point: the other members see the same records.  LDP: uploading the training
// set resets every member's QP list to the four slots, as the solo upload does.
static void share_set(ethcnn_train_group* g, int set, bool installed) {
    const ethcnn_trainer* t0 = g->m[0];
    for (size_t i = 1; i < g->m.size(); ++i) {
        ethcnn_trainer* t = g->m[i];
        t->data[set] = t0->data[set];
        t->nrec[set] = t0->nrec[set];
        std::memcpy(t->slot_of_qp[set], t0->slot_of_qp[set], sizeof t->slot_of_qp[set]);
        std::memcpy(t->slot_qps[set], t0->slot_qps[set], sizeof t->slot_qps[set]);
        if (installed && g->net == kNetLdp && set == ETHCNN_TRAIN_SET_TRAIN) {
            std::memcpy(t->qps, t0->qps, sizeof t->qps);
            t->nqps = t0->nqps;
        }
    }
    g->table_stale = true;
}

extern "C" int ethcnn_train_group_set_samples(ethcnn_train_group* g, int set, const uint8_t* rec, size_t nbytes) {
    if (!g) return ETHCNN_ERR_ARG;
    const int rc = ethcnn_train_set_samples(g->m[0], set, rec, nbytes);  // one copy, one slot-QP pass
    if (set == 0 || set == 1) share_set(g, set, rc == 0);
    if (rc) g->err = g->m[0]->err;
    return rc;
}

extern "C" int ethcnn_train_group_set_samples_from(ethcnn_train_group* g, int set, ethcnn_samples* sm, int take) {
    if (!g) return ETHCNN_ERR_ARG;
    const int rc = ethcnn_train_set_samples_from(g->m[0], set, sm, take);
    if (set == 0 || set == 1) share_set(g, set, rc == 0);
    if (rc) g->err = g->m[0]->err;
    return rc;
}

extern "C" int ethcnn_train_group_set_qps(ethcnn_train_group* g, int i, const int* qps, int n) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = member_index(g, i)) return rc;
    if (int rc = from_member(g, i, ethcnn_train_set_qps(g->m[(size_t)i], qps, n))) return rc;
    g->table_stale = true;
    return 0;
}

extern "C" int ethcnn_train_group_run(ethcnn_train_group* g, int64_t first_step, int64_t nsteps) {
    if (!g) return ETHCNN_ERR_ARG;
    if (first_step < 0 || nsteps < 0) return gerr(g, ETHCNN_ERR_ARG, "negative step");
    if (int rc = ready(g)) return rc;
    GCHK(g, hipSetDevice(g->c->device));
    if (int rc = upload_table(g)) return rc;
    for (int64_t i = 0; i < nsteps; ++i)
        if (int rc = enqueue_step(g, first_step + i, false)) return rc;
    return 0;
}

extern "C" int ethcnn_train_group_last_stats(ethcnn_train_group* g, float* loss, float* acc) {
    if (!g) return ETHCNN_ERR_ARG;
    GCHK(g, hipSetDevice(g->c->device));
    return read_stats(g, loss, acc);
}

extern "C" int ethcnn_train_group_step_indices(ethcnn_train_group* g, int64_t step, const int32_t* idx, const int* qp, int n, float* loss,
                                               float* acc) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = ready(g)) return rc;
    if (!idx || !qp || n != g->B) return gerr(g, ETHCNN_ERR_ARG, "an explicit batch needs %d indices and QPs per member", g->B);
    if (step < 0) return gerr(g, ETHCNN_ERR_ARG, "negative step");
    const ethcnn_trainer* t0 = g->m[0];
    for (int i = 0; i < g->K * n; ++i) {
        if (idx[i] < 0 || idx[i] >= t0->nrec[0])
            return gerr(g, ETHCNN_ERR_ARG, "member %d: sample index %d outside 0..%lld", i / n, idx[i], (long long)t0->nrec[0] - 1);
        if (qp[i] < 0 || qp[i] > 51) return gerr(g, ETHCNN_ERR_ARG, "member %d: QP %d outside 0..51", i / n, qp[i]);
        if (g->net == kNetLdp && t0->slot_of_qp[ETHCNN_TRAIN_SET_TRAIN][qp[i]] < 0)
            return gerr(g, ETHCNN_ERR_ARG, "member %d: QP %d is not a slot QP of the training samples", i / n, qp[i]);
    }
    GCHK(g, hipSetDevice(g->c->device));
    if (int rc = upload_table(g)) return rc;
    hipStream_t s = g->c->stream;
    for (int i = 0; i < g->K; ++i) {
        GCHK(g, hipMemcpyAsync(g->m[(size_t)i]->idx_in, idx + (size_t)i * n, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
        GCHK(g, hipMemcpyAsync(g->m[(size_t)i]->qp_in, qp + (size_t)i * n, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    }
    GCHK(g, hipStreamSynchronize(s));
    if (int rc = enqueue_step(g, step, true)) return rc;
    return read_stats(g, loss, acc);
}

extern "C" int ethcnn_train_group_evaluate(ethcnn_train_group* g, int set, const int32_t* idx, int64_t n, const int* qps, float* loss,
                                           float* acc, float* probs) {
    if (!g) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return gerr(g, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    const ethcnn_trainer* t0 = g->m[0];
    if (!t0->data[set]) return gerr(g, ETHCNN_ERR_ARG, "no samples in set %d", set);
    if (!qps) return gerr(g, ETHCNN_ERR_ARG, "no QPs");
    const bool ldp = g->net == kNetLdp;
    const int K = g->K;
    bool any_mixed = false;
    for (int i = 0; i < K; ++i) {
        const int qp = qps[i];
        if (!(qp >= 0 && qp <= 51) && !(ldp && qp == -1))
            return gerr(g, ETHCNN_ERR_ARG, ldp ? "member %d: QP %d is neither a slot QP nor -1" : "member %d: QP %d outside 0..51", i, qp);
        if (ldp && qp >= 0 && t0->slot_of_qp[set][qp] < 0) return gerr(g, ETHCNN_ERR_ARG, "member %d: QP %d is not a slot QP of set %d", i, qp, set);
        any_mixed = any_mixed || qp < 0;
    }
    if (n <= 0 || n > 0x7fffffffll || (!idx && n > t0->nrec[set])) return gerr(g, ETHCNN_ERR_ARG, "bad sample count %lld", (long long)n);
    if (idx)
        for (int64_t i = 0; i < n; ++i)
            if (idx[i] < 0 || idx[i] >= t0->nrec[set])
                return gerr(g, ETHCNN_ERR_ARG, "sample index %d outside 0..%lld", idx[i], (long long)t0->nrec[set] - 1);
    GCHK(g, hipSetDevice(g->c->device));
    hipStream_t s = g->c->stream;
    g->c->done_armed = 0;
    std::vector<int32_t> ids;
    if (!idx) {
        ids.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) ids[(size_t)i] = (int32_t)i;
        idx = ids.data();
    }
    // qp == -1: member m's sample i at the slot its own draw(2, 0, i, 0) picks among the four, as the solo evaluation
    std::vector<int32_t> mixed;
    if (any_mixed) {
        mixed.assign((size_t)K * (size_t)n, 0);
        for (int m = 0; m < K; ++m)
            if (qps[m] < 0)
                for (int64_t i = 0; i < n; ++i)
                    mixed[(size_t)m * n + i] = t0->slot_qps[set][((draw(g->m[(size_t)m]->opt.seed, kStreamQp, 0, (uint64_t)i, 0) >> 32) * 4ull) >> 32];
    }
    // one table per piece (launches 1-3) and one for the loss launch over all n
    const int64_t pieces = (n + g->cap - 1) / g->cap;
    float *Pn = nullptr, *Ln = nullptr;
    int32_t *In = nullptr, *Qn = nullptr;
    Member* d_tabs = nullptr;
    const auto release = [&]() { (void)hipFree(Pn); (void)hipFree(Ln); (void)hipFree(In); (void)hipFree(Qn); (void)hipFree(d_tabs); };
    if (hipMalloc((void**)&Pn, (size_t)K * n * kTOut * 4) != hipSuccess || hipMalloc((void**)&Ln, (size_t)K * n * 16 * 4) != hipSuccess ||
        hipMalloc((void**)&In, (size_t)n * 4) != hipSuccess || (any_mixed && hipMalloc((void**)&Qn, (size_t)K * n * 4) != hipSuccess) ||
        hipMalloc((void**)&d_tabs, sizeof(Member) * (size_t)K * (size_t)(pieces + 1)) != hipSuccess) {
        (void)hipGetLastError();
        release();
        return gerr(g, ETHCNN_ERR_NOMEM, "cannot allocate the evaluation buffers of %d x %lld samples", K, (long long)n);
    }
    std::vector<Member> tabs;
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
            tabs.push_back(e);
        }
    }
    hipError_t e = hipMemcpyAsync(In, idx, (size_t)n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && Qn) e = hipMemcpyAsync(Qn, mixed.data(), mixed.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tabs, tabs.data(), sizeof(Member) * tabs.size(), hipMemcpyHostToDevice, s);
    const NetOffsets& o = t0->o;
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
    if (e != hipSuccess) return gerr(g, ETHCNN_ERR_DEVICE, "evaluation: %s", hipGetErrorString(e));
    return read_stats(g, loss, acc);
}

extern "C" int ethcnn_train_group_debug_fetch(ethcnn_train_group* g, int i, int which, float* out, size_t nfloats) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = member_index(g, i)) return rc;
    return from_member(g, i, ethcnn_train_debug_fetch(g->m[(size_t)i], which, out, nfloats));
}
