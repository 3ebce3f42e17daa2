// ethcnn_lstm_train_group.cpp -- the step engine of ETH-LSTM training and the trainer group's entry points (include/ethcnn.h
// "ETH-LSTM training, several models at once").  The engine is K >= 1 trainers of ethcnn_lstm_train.cpp that share a context, a
// stream, the two sample sets and every launch of a step (kernels and grid mapping: ethcnn_lstm_train.h "the member table").  A
// trainer group is an engine over its K members; a solo trainer's entry points (ethcnn_lstm_train.cpp) call the ones below on an
// engine over the trainer itself, so there is one step, one evaluation and one sample validation.  Weights in and out, initialisation,
// the QP list and the debug buffers are the member's own business and go through its trainer entry points.  The engine holds ONE
// copy of each sample set and, per member, the list of the records its QP list keeps.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "ethcnn_ctx.h"
#include "ethcnn_lstm_samples.h"
#include "ethcnn_lstm_train.h"
#include "ethcnn_lstm_train_host.h"

using namespace ethcnn::lstm_train;
using ethcnn::kLstmBlobFloats;
using ethcnn::train::GemmGroup;
using ethcnn::train::GroupRates;
using ethcnn::train::kMaxMembers;
using ethcnn::train::launch_group_gemm;
using ethcnn::train::launch_group_loss;
typedef ethcnn::train::Member LossEntry;

static int from_member(ethcnn_lstm_train_group* g, int i, int rc) {
    if (rc) g->err = "member " + std::to_string(i) + ": " + g->m[(size_t)i]->err;
    return rc;
}
static int member_index(ethcnn_lstm_train_group* g, int i) {
    if (i < 0 || i >= g->K) return terr(g, ETHCNN_ERR_ARG, "member %d outside 0..%d", i, g->K - 1);
    return 0;
}
static const char* api(const ethcnn_lstm_train_group* g) { return g->group ? "ethcnn_lstm_train_group" : "ethcnn_lstm_train"; }

extern "C" int ethcnn_lstm_train_group_check(const ethcnn_lstm_train_options* opts, int k, char* err, size_t errcap) {
    char buf[256] = "";
    int rc = ETHCNN_OK;
    const auto fail = [&](const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        rc = ETHCNN_ERR_ARG;
    };
    if (k < 1 || k > kMaxMembers) fail("an LSTM trainer group holds 1..%d members, got k = %d", kMaxMembers, k);
    else if (!opts) fail("no options");
    for (int i = 0; rc == ETHCNN_OK && i < k; ++i) {
        const ethcnn_lstm_train_options& o = opts[i];
        if (o.batch <= 0 || o.batch > 4096) fail("member %d: batch must be in 1..4096, got %d", i, o.batch);
        else if (o.decay_steps <= 0) fail("member %d: decay_steps must be positive", i);
        else if (!std::isfinite(o.lr_init)) fail("member %d: lr_init is not finite", i);
        else if (!std::isfinite(o.momentum)) fail("member %d: momentum is not finite", i);
        else if (!std::isfinite(o.decay_rate)) fail("member %d: decay_rate is not finite", i);
        else if (!std::isfinite(o.qp_scale) || o.qp_scale < 0.f) fail("member %d: qp_scale must be finite and >= 0 (0 means 1.0)", i);
        else if (!std::isfinite(o.clip_norm) || o.clip_norm < 0.f) fail("member %d: clip_norm must be finite and >= 0 (0 means no clip)", i);
        else if (o.batch != opts[0].batch)
            fail("member %d: batch %d differs from member 0's %d (one batch size per group)", i, o.batch, opts[0].batch);
    }
    if (err && errcap) std::snprintf(err, errcap, "%s", buf);
    return rc;
}

// SELECT_QP_LIST on slot-0 QP floats: the records a member with this QP list keeps, in file order (nqps == 0: all)
static void select_qp(const float* q0, size_t n, const int* qps, int nqps, std::vector<int64_t>* keep) {
    keep->clear();
    for (size_t i = 0; i < n; ++i) {
        bool on = nqps == 0;
        for (int k = 0; k < nqps && !on; ++k) on = q0[i] == (float)qps[k];
        if (on) keep->push_back((int64_t)i);
    }
}

extern "C" int ethcnn_lstm_train_group_keep_list(const uint8_t* rec, size_t nbytes, const int* qps, int nqps, int64_t* keep, int64_t* nkept) {
    if (!nkept || nqps < 0 || nqps > 52 || (nqps > 0 && !qps) || (nbytes && !rec)) return ETHCNN_ERR_ARG;
    if (nbytes % kRecBytes) return ETHCNN_ERR_FORMAT;
    const size_t n = nbytes / kRecBytes;
    std::vector<float> q0(n);
    for (size_t i = 0; i < n; ++i) std::memcpy(&q0[i], rec + i * kRecBytes + 64, 4);
    std::vector<int64_t> k;
    select_qp(q0.data(), n, qps, nqps, &k);
    if (keep && !k.empty()) std::memcpy(keep, k.data(), k.size() * sizeof(int64_t));
    *nkept = (int64_t)k.size();
    return ETHCNN_OK;
}

// the tables of a training step, from the members and the sets as they are now
static LstmMember member_entry(const ethcnn_lstm_train_group* g, int i) {
    const ethcnn_lstm_trainer* t = g->m[(size_t)i];
    LstmMember e{};
    e.u = t->u;
    e.W = t->W; e.acc = t->acc; e.grad = t->grad; e.part = t->part; e.stats = t->stats;
    e.idx_in = t->idx_in; e.idx = t->idx;
    for (int s = 0; s < 2; ++s) {
        e.keep[s] = g->d_keep[s][i];
        e.nkept[s] = (long)g->nkept[s][i];
    }
    e.seed = t->opt.seed;
    e.qp_scale = t->qp_scale;
    e.dropout = t->opt.dropout ? 1 : 0;
    e.momentum = t->opt.momentum;
    e.clip = t->opt.clip_norm;
    return e;
}
static LossEntry loss_entry(const LstmMember& m) {
    LossEntry e{};
    e.P = m.u.P; e.lab = m.u.lab; e.stats = m.stats; e.dZ3 = m.u.dZ3;
    return e;
}

static int upload_table(ethcnn_lstm_train_group* g) {
    if (!g->stale) return 0;
    std::vector<LstmMember> tab;
    std::vector<LossEntry> loss;
    for (int i = 0; i < g->K; ++i) {
        tab.push_back(member_entry(g, i));
        loss.push_back(loss_entry(tab.back()));
    }
    TCHK(g, hipStreamSynchronize(g->c->stream));  // steps in flight still read the old tables
    TCHK(g, hipMemcpy(g->d_tab, tab.data(), sizeof(LstmMember) * tab.size(), hipMemcpyHostToDevice));
    TCHK(g, hipMemcpy(g->d_loss, loss.data(), sizeof(LossEntry) * loss.size(), hipMemcpyHostToDevice));
    g->stale = false;
    return 0;
}

// launches 1-4 of nb samples per member
static void enqueue_forward(ethcnn_lstm_train_group* g, const LstmMember* tab, int set, int nb, uint64_t step, int drawn, int train,
                            const GemmGroup* grps, int tiles) {
    hipStream_t s = g->c->stream;
    const LstmOffsets& o = g->m[0]->o;
    LstmGroupStep a{};
    a.data = g->data[set];
    a.step = step;
    a.set = set;
    a.drawn = drawn;
    launch_group_gather(s, nb, g->K, tab, a);
    launch_group_gemm(s, grps, tiles, g->K);
    launch_group_fwd(s, nb, g->K, tab, o);
    launch_group_heads_fwd(s, nb, g->K, tab, o, step, train);
    for (ethcnn_lstm_trainer* t : g->m) t->last_rows = nb * kSteps;
}

static int enqueue_step(ethcnn_lstm_train_group* g, int64_t step, bool explicit_batch) {
    hipStream_t s = g->c->stream;
    const LstmOffsets& o = g->m[0]->o;
    g->c->done_armed = 0;  // the context's completion word does not cover these launches
    GroupRates r{};
    for (int i = 0; i < g->K; ++i) {
        const ethcnn_lstm_train_options& p = g->m[(size_t)i]->opt;
        r.lr[i] = ethcnn::train::lr_at(p.lr_init, p.decay_rate, p.decay_steps, step);
    }
    enqueue_forward(g, g->d_tab, ETHCNN_TRAIN_SET_TRAIN, g->B, (uint64_t)step, explicit_batch ? 0 : 1, 1, g->d_fwd, g->t_fwd);
    launch_group_loss(s, g->K, g->d_loss, g->B * kSteps, 1);
    launch_group_heads_bwd(s, g->B, g->K, g->d_tab, o);
    launch_group_bwd(s, g->B, g->K, g->d_tab, o);
    launch_group_gemm(s, g->d_bwd, g->t_bwd, g->K);
    launch_group_norm_update(s, g->K, g->d_tab, r, (long)kLstmBlobFloats);
    TCHK(g, hipGetLastError());
    return 0;
}

static int read_stats(ethcnn_lstm_train_group* g, float* loss, float* acc) {
    float* st[kMaxMembers];
    for (int i = 0; i < g->K; ++i) st[i] = g->m[(size_t)i]->stats;
    TCHK(g, ethcnn::train::read_stats(g->c->stream, st, g->K, loss, acc));
    return 0;
}

static int ready(ethcnn_lstm_train_group* g) {
    if (!g->data[ETHCNN_TRAIN_SET_TRAIN]) return terr(g, ETHCNN_ERR_ARG, "no training samples (%s_set_samples)", api(g));
    return 0;
}

static void free_set(ethcnn_lstm_train_group* g, int set) {
    if (g->data[set]) (void)hipFree(g->data[set]);
    g->data[set] = nullptr;
    for (int i = 0; i < kMaxMembers; ++i) {
        if (g->d_keep[set][i]) (void)hipFree(g->d_keep[set][i]);
        g->d_keep[set][i] = nullptr;
        g->nkept[set][i] = 0;
    }
    g->nall[set] = 0;
}

void lstm_engine_destroy(ethcnn_lstm_train_group* g) {
    if (!g) return;
    for (int s = 0; s < 2; ++s) free_set(g, s);
    (void)hipFree(g->d_tab);
    (void)hipFree(g->d_loss);
    (void)hipFree(g->d_fwd);
    (void)hipFree(g->d_bwd);
    (void)hipFree(g->d_eval);
    delete g;
}

int lstm_engine_create(ethcnn_ctx* c, const std::vector<ethcnn_lstm_trainer*>& members, bool group, ethcnn_lstm_train_group** out) {
    ethcnn_lstm_train_group* g = new (std::nothrow) ethcnn_lstm_train_group;
    if (!g) return set_err(c, ETHCNN_ERR_NOMEM, "out of memory");
    const int k = (int)members.size();
    g->c = c;
    g->m = members;
    g->K = k;
    g->B = members[0]->B;
    g->cap = members[0]->cap;
    g->group = group;
    std::vector<GemmGroup> gf, gb, ge;
    for (const ethcnn_lstm_trainer* t : g->m) {
        gf.push_back(lstm_proj_group(t, g->B * kSteps));
        gb.push_back(lstm_grad_group(t, g->B * kSteps));
        ge.push_back(lstm_proj_group(t, g->cap * kSteps));
    }
    g->t_fwd = gf[0].tiles; g->t_bwd = gb[0].tiles; g->t_eval = ge[0].tiles;
    const size_t gbytes = sizeof(GemmGroup) * (size_t)k;
    hipError_t e = hipMalloc((void**)&g->d_tab, sizeof(LstmMember) * (size_t)k);
    e = e ? e : hipMalloc((void**)&g->d_loss, sizeof(LossEntry) * (size_t)k);
    e = e ? e : hipMalloc((void**)&g->d_fwd, gbytes);
    e = e ? e : hipMalloc((void**)&g->d_bwd, gbytes);
    e = e ? e : hipMalloc((void**)&g->d_eval, gbytes);
    e = e ? e : hipMemcpy(g->d_fwd, gf.data(), gbytes, hipMemcpyHostToDevice);
    e = e ? e : hipMemcpy(g->d_bwd, gb.data(), gbytes, hipMemcpyHostToDevice);
    e = e ? e : hipMemcpy(g->d_eval, ge.data(), gbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        lstm_engine_destroy(g);
        return set_err(c, ETHCNN_ERR_DEVICE, "LSTM %s setup: %s", group ? "trainer group" : "trainer", hipGetErrorString(e));
    }
    for (ethcnn_lstm_trainer* t : g->m) t->eng = g;
    *out = g;
    return ETHCNN_OK;
}

extern "C" void ethcnn_lstm_train_group_destroy(ethcnn_lstm_train_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->c->device);
    (void)hipStreamSynchronize(g->c->stream);
    for (ethcnn_lstm_trainer* t : g->m) lstm_member_destroy(t);
    lstm_engine_destroy(g);
}

extern "C" int ethcnn_lstm_train_group_create(ethcnn_ctx* c, const ethcnn_lstm_train_options* opts, int k, ethcnn_lstm_train_group** out) {
    if (!c || !out) return ETHCNN_ERR_ARG;
    *out = nullptr;
    char why[256];
    if (int rc = ethcnn_lstm_train_group_check(opts, k, why, sizeof why)) return set_err(c, rc, "%s", why);
    std::vector<ethcnn_lstm_trainer*> m;
    int rc = 0;
    for (int i = 0; i < k && !rc; ++i) {
        ethcnn_lstm_trainer* t = nullptr;
        rc = lstm_member_create(c, &opts[i], &t);  // (the context holds the message)
        if (!rc) m.push_back(t);
    }
    rc = rc ? rc : lstm_engine_create(c, m, true, out);
    if (rc)
        for (ethcnn_lstm_trainer* t : m) lstm_member_destroy(t);
    return rc;
}

extern "C" const char* ethcnn_lstm_train_group_last_error(const ethcnn_lstm_train_group* g) {
    return g ? g->err.c_str() : "LSTM trainer group is NULL";
}

extern "C" int ethcnn_lstm_train_group_init_weights(ethcnn_lstm_train_group* g, const uint64_t* seeds) {
    if (!g) return ETHCNN_ERR_ARG;
    if (!seeds) return terr(g, ETHCNN_ERR_ARG, "no seeds");
    for (int i = 0; i < g->K; ++i)
        if (int rc = from_member(g, i, ethcnn_lstm_train_init_weights(g->m[(size_t)i], seeds[i]))) return rc;
    return 0;
}

extern "C" int ethcnn_lstm_train_group_set_blob(ethcnn_lstm_train_group* g, int i, const float* blob, const float* accum, size_t n) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = member_index(g, i)) return rc;
    return from_member(g, i, ethcnn_lstm_train_set_blob(g->m[(size_t)i], blob, accum, n));
}

extern "C" int ethcnn_lstm_train_group_get_blob(ethcnn_lstm_train_group* g, int i, float* blob, float* accum, size_t n) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = member_index(g, i)) return rc;
    return from_member(g, i, ethcnn_lstm_train_get_blob(g->m[(size_t)i], blob, accum, n));
}

extern "C" int ethcnn_lstm_train_group_set_qps(ethcnn_lstm_train_group* g, int i, const int* qps, int n) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = member_index(g, i)) return rc;
    return from_member(g, i, ethcnn_lstm_train_set_qps(g->m[(size_t)i], qps, n));
}

// Installs `p` (nall records, already in HBM; `file_index`: the file record behind each of them, NULL = itself) as set `set` with the
// members' keep lists `keep` (indices into p).  Before that, the device validation over the records at least one member keeps; a bad
// record fails the upload for the first member that keeps one, with that member's first.
// On any failure p is NOT freed and the engine is unchanged.
static int install_set(ethcnn_lstm_train_group* g, int set, uint8_t* p, size_t nall, const int64_t* file_index,
                       std::vector<std::vector<int64_t>>& keep) {
    hipStream_t s = g->c->stream;
    const int K = g->K;
    std::vector<uint8_t> used(nall, 0);
    for (int i = 0; i < K; ++i)
        for (int64_t r : keep[(size_t)i]) used[(size_t)r] = 1;
    std::vector<int64_t> list;
    for (size_t r = 0; r < nall; ++r)
        if (used[r]) list.push_back((int64_t)r);
    const size_t nl = list.size();
    std::vector<uint8_t> bad(nl);
    {
        int64_t* d_list = nullptr;
        uint8_t* d_bad = nullptr;
        hipError_t e = hipMalloc((void**)&d_bad, nl);
        if (e == hipSuccess && nl != nall) e = hipMalloc((void**)&d_list, nl * 8);
        if (e == hipSuccess && d_list) e = hipMemcpyAsync(d_list, list.data(), nl * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            launch_check_list(s, p, d_list, (long)nl, d_bad, (int)std::min<size_t>(4096, nl));
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(bad.data(), d_bad, nl, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(d_list);
        (void)hipFree(d_bad);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return terr(g, ETHCNN_ERR_DEVICE, "sample check: %s", hipGetErrorString(e));
        }
    }
    for (size_t j = 0; j < nl; ++j) used[(size_t)list[j]] = bad[j] ? 2 : 1;
    for (int i = 0; i < K; ++i)
        for (int64_t r : keep[(size_t)i])
            if (used[(size_t)r] == 2)
                return gerr(g, i, ETHCNN_ERR_FORMAT, "sample %lld: a QP outside 0..51, a label outside 0..3 or a non-finite vector element",
                            (long long)(file_index ? file_index[r] : r));
    // the keep lists in HBM (a member that keeps everything reads the records directly)
    int64_t* d_keep[kMaxMembers] = {};
    for (int i = 0; i < K; ++i) {
        const std::vector<int64_t>& k = keep[(size_t)i];
        if (k.size() == nall) continue;
        hipError_t e = hipMalloc((void**)&d_keep[i], k.size() * 8);
        if (e == hipSuccess) e = hipMemcpy(d_keep[i], k.data(), k.size() * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            for (int j = 0; j <= i; ++j) (void)hipFree(d_keep[j]);
            return terr(g, ETHCNN_ERR_NOMEM, "cannot allocate a keep list of %zu samples", k.size());
        }
    }
    free_set(g, set);
    g->data[set] = p;
    g->nall[set] = (int64_t)nall;
    for (int i = 0; i < K; ++i) {
        g->d_keep[set][i] = d_keep[i];
        g->nkept[set][i] = (int64_t)keep[(size_t)i].size();
    }
    g->stale = true;
    return 0;
}

// the members' keep lists over n records with the slot-0 QPs q0; an empty one is an error
static int member_keeps(ethcnn_lstm_train_group* g, const float* q0, size_t n, std::vector<std::vector<int64_t>>* keep) {
    keep->assign((size_t)g->K, std::vector<int64_t>());
    for (int i = 0; i < g->K; ++i) {
        const ethcnn_lstm_trainer* t = g->m[(size_t)i];
        select_qp(q0, n, t->qps, t->nqps, &(*keep)[(size_t)i]);
        if ((*keep)[(size_t)i].empty()) return gerr(g, i, ETHCNN_ERR_FORMAT, "none of the %zu samples has a selected QP", n);
        if ((*keep)[(size_t)i].size() > 0x7fffffffull / kSteps) return gerr(g, i, ETHCNN_ERR_ARG, "too many samples");
    }
    return 0;
}

extern "C" int ethcnn_lstm_train_group_set_samples(ethcnn_lstm_train_group* g, int set, const uint8_t* rec, size_t nbytes) {
    if (!g) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return terr(g, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    if (!rec || nbytes == 0) return terr(g, ETHCNN_ERR_ARG, "no sample records");
    if (nbytes % kRecBytes) return terr(g, ETHCNN_ERR_FORMAT, "%zu bytes is not a whole number of %d-byte samples", nbytes, kRecBytes);
    const size_t nfile = nbytes / kRecBytes;
    std::vector<float> q0(nfile);
    for (size_t i = 0; i < nfile; ++i) std::memcpy(&q0[i], rec + i * kRecBytes + 64, 4);
    std::vector<std::vector<int64_t>> keep;
    if (int rc = member_keeps(g, q0.data(), nfile, &keep)) return rc;
    // only the records some member keeps go to HBM: `un` lists them (file order), pos[r] = where file record r lies in the copy
    std::vector<int64_t> pos(nfile, -1), un;
    for (const std::vector<int64_t>& k : keep)
        for (int64_t r : k) pos[(size_t)r] = 0;
    for (size_t r = 0; r < nfile; ++r)
        if (pos[r] == 0) {
            pos[r] = (int64_t)un.size();
            un.push_back((int64_t)r);
        }
    for (std::vector<int64_t>& k : keep)
        for (int64_t& r : k) r = pos[(size_t)r];
    TCHK(g, hipSetDevice(g->c->device));
    TCHK(g, hipStreamSynchronize(g->c->stream));
    const size_t n = un.size();
    void* p = nullptr;
    if (hipMalloc(&p, n * kRecBytes) != hipSuccess) {
        (void)hipGetLastError();
        return terr(g, ETHCNN_ERR_NOMEM, "%zu bytes of samples do not fit in device memory", n * kRecBytes);
    }
    hipError_t e = hipSuccess;
    for (size_t j = 0; j < n && e == hipSuccess;) {  // runs of consecutive records, one copy each
        size_t k = j + 1;
        while (k < n && un[k] == un[k - 1] + 1) ++k;
        e = hipMemcpy((uint8_t*)p + j * kRecBytes, rec + (size_t)un[j] * kRecBytes, (k - j) * kRecBytes, hipMemcpyHostToDevice);
        j = k;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(p);
        return terr(g, ETHCNN_ERR_DEVICE, "sample upload: %s", hipGetErrorString(e));
    }
    if (int rc = install_set(g, set, (uint8_t*)p, n, un.data(), keep)) {
        (void)hipFree(p);
        return rc;
    }
    return 0;
}

extern "C" int ethcnn_lstm_train_group_set_samples_from(ethcnn_lstm_train_group* g, int set, ethcnn_lstm_samples* sm, int take) {
    namespace ls = ethcnn::lstm_samples;
    if (!g) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return terr(g, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    if (!sm || !sm->built || sm->count == 0) return terr(g, ETHCNN_ERR_ARG, "no sample records (the sample set is not built or empty)");
    if (sm->c != g->c)
        return terr(g, ETHCNN_ERR_ARG, "the sample set and the trainer%s live on different contexts", g->group ? " group" : "");
    const size_t nall = (size_t)sm->count;
    hipStream_t s = g->c->stream;
    TCHK(g, hipSetDevice(g->c->device));
    TCHK(g, hipStreamSynchronize(s));
    bool selecting = false;  // some member has a QP list: the slot-0 QPs are the only bytes that leave HBM
    for (const ethcnn_lstm_trainer* t : g->m) selecting = selecting || t->nqps > 0;
    std::vector<float> q0(selecting ? nall : 0);
    if (selecting) {
        float* d_q = nullptr;
        hipError_t e = hipMalloc((void**)&d_q, nall * 4);
        if (e == hipSuccess) {
            ls::launch_qp0(s, sm->data, (long)nall, d_q);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(q0.data(), d_q, nall * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(d_q);
        if (e != hipSuccess) return terr(g, ETHCNN_ERR_DEVICE, "sample selection: %s", hipGetErrorString(e));
    }
    std::vector<std::vector<int64_t>> keep;
    if (int rc = member_keeps(g, q0.data(), nall, &keep)) return rc;
    // A trainer group keeps the whole set once and reads it through the keep lists.  A solo trainer holds only the records it keeps:
    // under a QP list that drops some, a compacted copy with everything kept (`file`: the set's record behind each of its records).
    const bool compact = !g->group && keep[0].size() != nall;
    std::vector<int64_t> file;
    if (compact) {
        file.swap(keep[0]);
        keep[0].resize(file.size());
        std::iota(keep[0].begin(), keep[0].end(), (int64_t)0);
    }
    const size_t n = compact ? file.size() : nall;
    const bool copy = compact || !take;  // otherwise the set's buffer is adopted
    uint8_t* p = sm->data;
    if (copy) {
        if (hipMalloc((void**)&p, n * kRecBytes) != hipSuccess) {
            (void)hipGetLastError();
            return terr(g, ETHCNN_ERR_NOMEM, "%zu bytes of samples do not fit in device memory", n * kRecBytes);
        }
        hipError_t e = hipSuccess;
        int64_t* d_file = nullptr;
        if (!compact) {
            e = hipMemcpyAsync(p, sm->data, n * kRecBytes, hipMemcpyDeviceToDevice, s);
        } else {
            e = hipMalloc((void**)&d_file, n * 8);
            if (e == hipSuccess) e = hipMemcpyAsync(d_file, file.data(), n * 8, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) {
                ls::launch_compact(s, sm->data, d_file, (long)n, p, g->c->cus > 0 ? g->c->cus : 256);
                e = hipGetLastError();
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(d_file);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(p);
            return terr(g, ETHCNN_ERR_DEVICE, "sample copy: %s", hipGetErrorString(e));
        }
    }
    if (int rc = install_set(g, set, p, n, compact ? file.data() : nullptr, keep)) {
        if (copy) (void)hipFree(p);
        return rc;
    }
    if (take) {  // the set is empty afterwards: its buffer is the engine's now, or (after a compacting copy) is freed
        if (copy) (void)hipFree(sm->data);
        sm->data = nullptr;
        sm->count = sm->skipped = 0;
        sm->built = false;
    }
    return 0;
}

extern "C" int64_t ethcnn_lstm_train_group_num_samples(const ethcnn_lstm_train_group* g, int i, int set) {
    return (g && i >= 0 && i < g->K && (set == 0 || set == 1)) ? g->nkept[set][i] : -1;
}

extern "C" int ethcnn_lstm_train_group_run(ethcnn_lstm_train_group* g, int64_t first_step, int64_t nsteps) {
    if (!g) return ETHCNN_ERR_ARG;
    if (first_step < 0 || nsteps < 0) return terr(g, ETHCNN_ERR_ARG, "negative step");
    if (int rc = ready(g)) return rc;
    TCHK(g, hipSetDevice(g->c->device));
    if (int rc = upload_table(g)) return rc;
    for (int64_t i = 0; i < nsteps; ++i)
        if (int rc = enqueue_step(g, first_step + i, false)) return rc;
    return 0;
}

extern "C" int ethcnn_lstm_train_group_last_stats(ethcnn_lstm_train_group* g, float* loss, float* acc) {
    if (!g) return ETHCNN_ERR_ARG;
    TCHK(g, hipSetDevice(g->c->device));
    return read_stats(g, loss, acc);
}

extern "C" int ethcnn_lstm_train_group_step_indices(ethcnn_lstm_train_group* g, int64_t step, const int32_t* idx, int n, float* loss,
                                                    float* acc) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = ready(g)) return rc;
    if (!idx || n != g->B) return terr(g, ETHCNN_ERR_ARG, "an explicit batch needs %d indices%s", g->B, g->group ? " per member" : "");
    if (step < 0) return terr(g, ETHCNN_ERR_ARG, "negative step");
    for (int i = 0; i < g->K * n; ++i)
        if (idx[i] < 0 || idx[i] >= g->nkept[0][i / n])
            return gerr(g, i / n, ETHCNN_ERR_ARG, "sample index %d outside 0..%lld", idx[i], (long long)g->nkept[0][i / n] - 1);
    TCHK(g, hipSetDevice(g->c->device));
    if (int rc = upload_table(g)) return rc;
    hipStream_t s = g->c->stream;
    for (int i = 0; i < g->K; ++i)
        TCHK(g, hipMemcpyAsync(g->m[(size_t)i]->idx_in, idx + (size_t)i * n, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    TCHK(g, hipStreamSynchronize(s));
    if (int rc = enqueue_step(g, step, true)) return rc;
    return read_stats(g, loss, acc);
}

extern "C" int ethcnn_lstm_train_group_evaluate(ethcnn_lstm_train_group* g, int set, const int32_t* idx, int64_t n, float* loss, float* acc,
                                                float* probs) {
    if (!g) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return terr(g, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    if (!g->data[set]) return terr(g, ETHCNN_ERR_ARG, "no samples in set %d", set);
    const int K = g->K;
    if (n <= 0 || n > 0x7fffffffll / kOut / kSteps / K) return terr(g, ETHCNN_ERR_ARG, "bad sample count %lld", (long long)n);
    for (int m = 0; m < K; ++m) {
        const int64_t cnt = g->nkept[set][m];
        if (!idx && n > cnt) {
            if (!g->group) return terr(g, ETHCNN_ERR_ARG, "bad sample count %lld", (long long)n);
            return gerr(g, m, ETHCNN_ERR_ARG, "bad sample count %lld (it keeps %lld)", (long long)n, (long long)cnt);
        }
        if (idx)
            for (int64_t i = 0; i < n; ++i)
                if (idx[m * n + i] < 0 || idx[m * n + i] >= cnt)
                    return gerr(g, m, ETHCNN_ERR_ARG, "sample index %d outside 0..%lld", idx[m * n + i], (long long)cnt - 1);
    }
    TCHK(g, hipSetDevice(g->c->device));
    hipStream_t s = g->c->stream;
    g->c->done_armed = 0;
    std::vector<int32_t> ids;
    if (!idx) {
        ids.resize((size_t)K * (size_t)n);
        for (int m = 0; m < K; ++m)
            for (int64_t i = 0; i < n; ++i) ids[(size_t)m * n + i] = (int32_t)i;
        idx = ids.data();
    }
    // one member table per piece (launches 1-4) and one loss table for the single loss launch over all 20 n rows of each member.
    // Tables and indices share ONE allocation and ONE upload, staged in `host`: [member tables | loss table | indices].
    const int64_t pieces = (n + g->cap - 1) / g->cap;
    const size_t rows = (size_t)n * kSteps;
    const size_t tab_bytes = sizeof(LstmMember) * (size_t)K * (size_t)pieces, loss_bytes = sizeof(LossEntry) * (size_t)K;
    const size_t in_bytes = (size_t)K * (size_t)n * 4;
    float *Pn = nullptr, *Ln = nullptr;
    uint8_t* D = nullptr;
    const auto release = [&]() { (void)hipFree(Pn); (void)hipFree(Ln); (void)hipFree(D); };
    if (hipMalloc((void**)&Pn, (size_t)K * rows * kOut * 4) != hipSuccess || hipMalloc((void**)&Ln, (size_t)K * rows * 16 * 4) != hipSuccess ||
        hipMalloc((void**)&D, tab_bytes + loss_bytes + in_bytes) != hipSuccess) {
        (void)hipGetLastError();
        release();
        return terr(g, ETHCNN_ERR_NOMEM, "cannot allocate the evaluation buffers of %d x %lld samples", K, (long long)n);
    }
    LstmMember* d_tabs = (LstmMember*)D;
    LossEntry* d_loss = (LossEntry*)(D + tab_bytes);
    int32_t* In = (int32_t*)(D + tab_bytes + loss_bytes);
    std::vector<uint8_t> host(tab_bytes + loss_bytes + in_bytes);
    LstmMember* tabs = (LstmMember*)host.data();
    LossEntry* losses = (LossEntry*)(host.data() + tab_bytes);
    for (int64_t p = 0; p < pieces; ++p) {
        const int64_t c0 = p * g->cap;
        for (int m = 0; m < K; ++m) {
            LstmMember e = member_entry(g, m);
            e.idx_in = In + (size_t)m * n + c0;
            e.u.P = Pn + ((size_t)m * rows + (size_t)c0 * kSteps) * kOut;
            e.u.lab = Ln + ((size_t)m * rows + (size_t)c0 * kSteps) * 16;
            tabs[p * K + m] = e;
        }
    }
    for (int m = 0; m < K; ++m) {
        LossEntry e{};
        e.P = Pn + (size_t)m * rows * kOut;
        e.lab = Ln + (size_t)m * rows * 16;
        e.stats = g->m[(size_t)m]->stats;
        losses[m] = e;
    }
    std::memcpy(host.data() + tab_bytes + loss_bytes, idx, in_bytes);
    hipError_t e = hipMemcpyAsync(D, host.data(), host.size(), hipMemcpyHostToDevice, s);  // (`host` lives until the last synchronisation)
    for (int64_t p = 0; e == hipSuccess && p < pieces; ++p) {
        const int nb = (int)std::min<int64_t>(g->cap, n - p * g->cap);
        enqueue_forward(g, d_tabs + p * K, set, nb, 0, 0, 0, g->d_eval, g->t_eval);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        launch_group_loss(s, K, d_loss, (int)rows, 0);  // per member ONE batch over all n x 20 rows
        e = hipGetLastError();
    }
    if (e == hipSuccess && probs) e = hipMemcpyAsync(probs, Pn, (size_t)K * rows * kOut * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    release();
    if (e != hipSuccess) return terr(g, ETHCNN_ERR_DEVICE, "evaluation: %s", hipGetErrorString(e));
    return read_stats(g, loss, acc);
}

extern "C" int ethcnn_lstm_train_group_debug_fetch(ethcnn_lstm_train_group* g, int i, int which, float* out, size_t nfloats) {
    if (!g) return ETHCNN_ERR_ARG;
    if (int rc = member_index(g, i)) return rc;
    return from_member(g, i, ethcnn_lstm_train_debug_fetch(g->m[(size_t)i], which, out, nfloats));
}

extern "C" int64_t ethcnn_lstm_train_group_debug_rows(const ethcnn_lstm_train_group* g, int i) {
    return (g && i >= 0 && i < g->K) ? g->m[(size_t)i]->last_rows : -1;
}
