// ethcnn_train.cpp -- host side of the trainer (include/ethcnn.h "training"): buffers, the GEMM descriptor tables, the step and
// evaluation sequences (kernels: ethcnn_train_kernels.hip, launch order: ethcnn_train.h).
#include <algorithm>
#include <cmath>
#include <new>
#include <cstring>
#include <string>
#include <vector>

#include "ethcnn_ctx.h"
#include "ethcnn_samples.h"
#include "ethcnn_train.h"
#include "ethcnn_train_host.h"

namespace ethcnn {
namespace train {
void launch_trunk_fwd(hipStream_t s, int nb, const StepArgs& a, const float* W, const NetOffsets& o, int net);
void launch_gemm(hipStream_t s, const GemmGroup* d_grp, int tiles);
void launch_heads_fwd(hipStream_t s, int nb, const float* Z1, float* A1, float* M1, float* H1, float* A2, float* M2, float* H2,
                      float* P, const int32_t* qp, const float* W, const NetOffsets& o, uint64_t seed, uint64_t step, int dropout, int net);
void launch_loss(hipStream_t s, const float* P, const float* lab, int n, float* stats, float* dZ);
void launch_heads_bwd(hipStream_t s, int nb, const float* dZ3, const float* A1, const float* M1, const float* A2, const float* M2,
                      float* dZ2, float* dZ1, const float* W, const NetOffsets& o, int dropout);
void launch_trunk_bwd(hipStream_t s, int nb, const float* trunk, const float* F, const float* dF, const float* W, const NetOffsets& o,
                      float* part);
void launch_update(hipStream_t s, float* W, float* acc, float* grad, const float* part, int nb, float lr, float momentum, long n,
                   const TuneMask& mask);
void launch_check_slots(hipStream_t s, const uint8_t* data, long nrec, uint32_t want, long* first_bad, int nblocks);
}  // namespace train
}  // namespace ethcnn

using namespace ethcnn::train;
using ethcnn::kBlobFloats;
using ethcnn::kNumTensors;
using ethcnn::kTensors;
using ethcnn::TensorDesc;

namespace {
constexpr int kEvalChunk = 1024;
const int kHN1[3] = {64, 128, 256}, kHN2[3] = {48, 96, 192}, kHN3[3] = {1, 4, 16};
const int kHOff1[3] = {0, 64, 192}, kHOff2[3] = {0, 48, 144}, kHOff3[3] = {0, 1, 5};
const int kH1Off[3] = {0, 66, 196}, kH2Off[3] = {0, 50, 148};
const char* kHeadTag[3] = {"64", "32", "16"};

int tensor_off(const char* name) {
    for (int t = 0; t < kNumTensors; ++t)
        if (std::strcmp(kTensors[t].name, name) == 0) return (int)(kTensors[t].offset_bytes / 4);
    return -1;
}
}  // namespace

static int terr(ethcnn_trainer* t, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t->err = buf;
    return code;
}
#define TCHK(t, call)                                                                                           \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess) return terr((t), ETHCNN_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

template <typename T>
static int talloc(ethcnn_trainer* t, T** p, size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 4) != hipSuccess) {
        (void)hipGetLastError();
        return terr(t, ETHCNN_ERR_NOMEM, "cannot allocate %zu bytes of device memory", count * sizeof(T));
    }
    t->allocs.push_back(q);
    *p = (T*)q;
    return 0;
}

static void add_desc(GemmGroup& g, GemmDesc d) {
    d.tiles_n = (d.N + 63) / 64;
    d.tile_begin = g.tiles;
    g.tiles += ((d.M + 63) / 64) * d.tiles_n;
    if (d.nseg == 0) {
        d.nseg = 1;
        d.kseg[0] = 0;
    }
    if (d.msplit == 0) d.msplit = d.M;
    g.d[g.n++] = d;
}

// FC1 forward of m rows: Z1[:, head] = F[:, :2688] x W1_head
GemmGroup train_fc1_group(const ethcnn_trainer* t, int m) {
    GemmGroup g{};
    for (int h = 0; h < 3; ++h) {
        GemmDesc d{};
        d.M = m; d.N = kHN1[h]; d.K = kTF;
        d.A = t->F; d.sam = kLdF; d.sak = 1;
        d.B[0] = t->W + t->o.w1[h]; d.sbk[0] = kHN1[h]; d.sbn[0] = 1;
        d.C = t->Z1 + kHOff1[h]; d.ldc = kTV;
        add_desc(g, d);
    }
    return g;
}

// dF = dZ1 x W1^T (K = 448 over the three heads' tensors) and the nine FC weight / bias gradients X_aug^T x dZ, written into grad
// (tune 1..3: only the tuned head's three GEMMs; the conv gradients have no reader, so dF is not formed)
GemmGroup train_bwd_group(const ethcnn_trainer* t, int m) {
    GemmGroup g{};
    if (!t->tune) {
        GemmDesc f{};
        f.M = m; f.N = kTF; f.K = kTV; f.nseg = 3;
        f.A = t->dZ1; f.sam = kTV; f.sak = 1;
        for (int h = 0; h < 3; ++h) {
            f.B[h] = t->W + t->o.w1[h]; f.sbk[h] = 1; f.sbn[h] = kHN1[h]; f.kseg[h] = kHOff1[h];
        }
        f.C = t->dF; f.ldc = kTF;
        add_desc(g, f);
    }
    for (int h = 0; h < 3; ++h) {
        if (t->tune && h != t->tune - 1) continue;
        GemmDesc d{};  // dW1 | db1: rows 0..2687 from F, row 2688 = the ones column
        d.M = kLdF; d.N = kHN1[h]; d.K = m; d.msplit = kTF;
        d.A = t->F; d.sam = 1; d.sak = kLdF;
        d.B[0] = t->dZ1 + kHOff1[h]; d.sbk[0] = kTV; d.sbn[0] = 1;
        d.C = t->grad + t->o.w1[h]; d.C2 = t->grad + t->o.b1[h]; d.ldc = kHN1[h];
        add_desc(g, d);
        GemmDesc e{};  // dW2 | db2 from [h1 (dropped), qp, 1]
        e.M = kHN1[h] + 2; e.N = kHN2[h]; e.K = m; e.msplit = kHN1[h] + 1;
        e.A = t->H1 + kH1Off[h]; e.sam = 1; e.sak = 454;
        e.B[0] = t->dZ2 + kHOff2[h]; e.sbk[0] = kT2; e.sbn[0] = 1;
        e.C = t->grad + t->o.w2[h]; e.C2 = t->grad + t->o.b2[h]; e.ldc = kHN2[h];
        add_desc(g, e);
        GemmDesc y{};  // dW3 | db3 from [h2 (dropped), qp, 1]
        y.M = kHN2[h] + 2; y.N = kHN3[h]; y.K = m; y.msplit = kHN2[h] + 1;
        y.A = t->H2 + kH2Off[h]; y.sam = 1; y.sak = 342;
        y.B[0] = t->dZ3 + kHOff3[h]; y.sbk[0] = kTOut; y.sbn[0] = 1;
        y.C = t->grad + t->o.w3[h]; y.C2 = t->grad + t->o.b3[h]; y.ldc = kHN3[h];
        add_desc(g, y);
    }
    return g;
}

float train_lr_at(const ethcnn_trainer* t, int64_t step) {  // tf.train.exponential_decay(..., staircase=True)
    const double p = std::floor((double)step / (double)t->opt.decay_steps);
    return (float)((double)t->opt.lr_init * std::pow((double)t->opt.decay_rate, p));
}

// trunk forward .. heads forward of nb rows (evaluation and training share it)
static void enqueue_forward(ethcnn_trainer* t, int set, int nb, const int32_t* d_idx, const int32_t* d_qp, int qp_fixed, uint64_t step,
                            int dropout, float* P, float* lab, const GemmGroup* grp, int tiles) {
    hipStream_t s = t->c->stream;
    StepArgs a{};
    a.data = t->data[set];
    a.nrec = t->nrec[set];
    a.idx_in = d_idx;
    a.qp_in = d_qp;
    std::memcpy(a.qps, t->qps, sizeof a.qps);
    a.nqps = t->nqps;
    a.qp_fixed = qp_fixed;
    std::memcpy(a.slot_of_qp, t->slot_of_qp[set], sizeof a.slot_of_qp);
    a.seed = t->opt.seed;
    a.step = step;
    a.dropout = dropout;
    a.idx_out = t->idx;
    a.qp_out = t->qp;
    a.labels = lab;
    a.trunk = t->trunk;
    a.F = t->F;
    launch_trunk_fwd(s, nb, a, t->W, t->o, t->net);
    launch_gemm(s, grp, tiles);
    launch_heads_fwd(s, nb, t->Z1, t->A1, t->M1, t->H1, t->A2, t->M2, t->H2, P, t->qp, t->W, t->o, t->opt.seed, step, dropout, t->net);
}

static int enqueue_step(ethcnn_trainer* t, int64_t step, bool explicit_batch) {
    hipStream_t s = t->c->stream;
    t->c->done_armed = 0;  // the context's completion word does not cover these launches
    const int dropout = t->opt.dropout ? 1 : 0;
    enqueue_forward(t, ETHCNN_TRAIN_SET_TRAIN, t->B, explicit_batch ? t->idx_in : nullptr, explicit_batch ? t->qp_in : nullptr, -1,
                    (uint64_t)step, dropout, t->P, t->lab, t->g_fwd, t->t_fwd);
    launch_loss(s, t->P, t->lab, t->B, t->stats, t->dZ3);
    launch_heads_bwd(s, t->B, t->dZ3, t->A1, t->M1, t->A2, t->M2, t->dZ2, t->dZ1, t->W, t->o, dropout);
    launch_gemm(s, t->g_bwd, t->t_bwd);
    if (!t->tune) launch_trunk_bwd(s, t->B, t->trunk, t->F, t->dF, t->W, t->o, t->part);
    launch_update(s, t->W, t->acc, t->grad, t->part, t->B, train_lr_at(t, step), t->opt.momentum, (long)kBlobFloats, t->mask);
    TCHK(t, hipGetLastError());
    return 0;
}

static int read_stats(ethcnn_trainer* t, float* loss3, float* acc3) {
    float st[8];
    TCHK(t, hipMemcpyAsync(st, t->stats, sizeof st, hipMemcpyDeviceToHost, t->c->stream));
    TCHK(t, hipStreamSynchronize(t->c->stream));
    for (int i = 0; i < 3; ++i) {
        if (loss3) loss3[i] = st[i];
        if (acc3) acc3[i] = st[3 + i];
    }
    return 0;
}

static int ready(ethcnn_trainer* t) {
    if (!t->data[ETHCNN_TRAIN_SET_TRAIN]) return terr(t, ETHCNN_ERR_ARG, "no training samples (ethcnn_train_set_samples)");
    if (!t->nqps) return terr(t, ETHCNN_ERR_ARG, "no QP list (ethcnn_train_set_qps)");
    return 0;
}

extern "C" int ethcnn_train_create(ethcnn_ctx* c, const ethcnn_train_options* opt, ethcnn_trainer** out) {
    if (!c || !opt || !out) return ETHCNN_ERR_ARG;
    *out = nullptr;
    if (opt->batch <= 0 || opt->batch > 65536) return set_err(c, ETHCNN_ERR_ARG, "batch must be in 1..65536, got %d", opt->batch);
    if (opt->decay_steps <= 0) return set_err(c, ETHCNN_ERR_ARG, "decay_steps must be positive");
    if (!std::isfinite(opt->lr_init) || !std::isfinite(opt->momentum) || !std::isfinite(opt->decay_rate))
        return set_err(c, ETHCNN_ERR_ARG, "non-finite optimiser option");
    if (opt->net != ETHCNN_TRAIN_NET_AI && opt->net != ETHCNN_TRAIN_NET_LDP)
        return set_err(c, ETHCNN_ERR_ARG, "net must be %d (All-Intra) or %d (LDP), got %d", ETHCNN_TRAIN_NET_AI, ETHCNN_TRAIN_NET_LDP, opt->net);
    if (opt->tune < 0 || opt->tune > 3) return set_err(c, ETHCNN_ERR_ARG, "tune must be in 0..3, got %d", opt->tune);
    if (hipSetDevice(c->device) != hipSuccess) return set_err(c, ETHCNN_ERR_DEVICE, "hipSetDevice(%d) failed", c->device);
    ethcnn_trainer* t = new (std::nothrow) ethcnn_trainer;
    if (!t) return set_err(c, ETHCNN_ERR_NOMEM, "out of memory");
    t->c = c;
    t->opt = *opt;
    t->B = opt->batch;
    t->cap = std::max(t->B, kEvalChunk);
    t->net = opt->net;
    t->tune = opt->tune;
    for (int s = 0; s < 2; ++s)
        for (int q = 0; q < 52; ++q) t->slot_of_qp[s][q] = -1;
    for (int br = 0; br < 3; ++br) {  // conv variables in creation order L, M, S (net_CTU64.py:122-138): Variable_{6 br' + 2 l}
        const int bc = br == 0 ? 2 : (br == 1 ? 1 : 0);
        for (int l = 0; l < 3; ++l) {
            char wn[32], bn[32];
            const int v = 6 * bc + 2 * l;
            if (v == 0) std::snprintf(wn, sizeof wn, "Variable");
            else std::snprintf(wn, sizeof wn, "Variable_%d", v);
            std::snprintf(bn, sizeof bn, "Variable_%d", v + 1);
            t->o.convw[br][l] = tensor_off(wn);
            t->o.convb[br][l] = tensor_off(bn);
        }
    }
    for (int h = 0; h < 3; ++h) {
        char n[40];
        const char* tag = kHeadTag[h];
        std::snprintf(n, sizeof n, "h_fc1__%s__w", tag); t->o.w1[h] = tensor_off(n);
        std::snprintf(n, sizeof n, "h_fc1__%s__b", tag); t->o.b1[h] = tensor_off(n);
        std::snprintf(n, sizeof n, "h_fc2__%s__w", tag); t->o.w2[h] = tensor_off(n);
        std::snprintf(n, sizeof n, "h_fc2__%s__b", tag); t->o.b2[h] = tensor_off(n);
        std::snprintf(n, sizeof n, "y_conv_flat__%s__w", tag); t->o.w3[h] = tensor_off(n);
        std::snprintf(n, sizeof n, "y_conv_flat__%s__b", tag); t->o.b3[h] = tensor_off(n);
    }
    if (t->tune) {  // PARTLY_TUNING_MODE (net_CTU64.py:200-209): the six tensors whose names hold __64__ / __32__ / __16__
        const int h = t->tune - 1, n1 = kHN1[h], n2 = kHN2[h], n3 = kHN3[h];
        const int off[6] = {t->o.w1[h], t->o.b1[h], t->o.w2[h], t->o.b2[h], t->o.w3[h], t->o.b3[h]};
        const int cnt[6] = {kTF * n1, n1, (n1 + 1) * n2, n2, (n2 + 1) * n3, n3};
        for (int i = 0; i < 6; ++i) {
            t->mask.lo[i] = off[i];
            t->mask.hi[i] = (long)off[i] + cnt[i];
        }
        t->mask.n = 6;
    }
    const size_t R = (size_t)t->cap;
    int rc = 0;
    rc = rc ? rc : talloc(t, &t->W, kBlobFloats);
    rc = rc ? rc : talloc(t, &t->acc, kBlobFloats);
    rc = rc ? rc : talloc(t, &t->grad, kBlobFloats);
    rc = rc ? rc : talloc(t, &t->idx, R);
    rc = rc ? rc : talloc(t, &t->qp, R);
    rc = rc ? rc : talloc(t, &t->idx_in, R);
    rc = rc ? rc : talloc(t, &t->qp_in, R);
    rc = rc ? rc : talloc(t, &t->lab, R * 16);
    rc = rc ? rc : talloc(t, &t->trunk, R * kTrunkRec);
    rc = rc ? rc : talloc(t, &t->F, R * kLdF);
    rc = rc ? rc : talloc(t, &t->Z1, R * kTV);
    rc = rc ? rc : talloc(t, &t->A1, R * kTV);
    rc = rc ? rc : talloc(t, &t->M1, R * kTV);
    rc = rc ? rc : talloc(t, &t->H1, R * 454);
    rc = rc ? rc : talloc(t, &t->A2, R * kT2);
    rc = rc ? rc : talloc(t, &t->M2, R * kT2);
    rc = rc ? rc : talloc(t, &t->H2, R * 342);
    rc = rc ? rc : talloc(t, &t->P, R * kTOut);
    rc = rc ? rc : talloc(t, &t->dZ3, R * kTOut);
    rc = rc ? rc : talloc(t, &t->dZ2, R * kT2);
    rc = rc ? rc : talloc(t, &t->dZ1, R * kTV);
    rc = rc ? rc : talloc(t, &t->dF, R * kTF);
    rc = rc ? rc : talloc(t, &t->part, (size_t)t->B * kConvFloats);
    rc = rc ? rc : talloc(t, &t->stats, 8);
    rc = rc ? rc : talloc(t, &t->g_fwd, 1);
    rc = rc ? rc : talloc(t, &t->g_bwd, 1);
    rc = rc ? rc : talloc(t, &t->g_eval, 1);
    if (rc) {
        const std::string why = t->err;
        ethcnn_train_destroy(t);
        return set_err(c, rc, "%s", why.c_str());
    }
    // zeroed once: rows past a short evaluation chunk are computed by the FC1 GEMM but never read
    hipError_t e = hipSuccess;
    for (void* p : {(void*)t->W, (void*)t->acc, (void*)t->grad}) e = e ? e : hipMemsetAsync(p, 0, kBlobFloats * 4, c->stream);
    e = e ? e : hipMemsetAsync(t->F, 0, R * kLdF * 4, c->stream);
    e = e ? e : hipMemsetAsync(t->stats, 0, 32, c->stream);
    const GemmGroup gf = train_fc1_group(t, t->B), gb = train_bwd_group(t, t->B), ge = train_fc1_group(t, t->cap);
    t->t_fwd = gf.tiles; t->t_bwd = gb.tiles; t->t_eval = ge.tiles;
    e = e ? e : hipMemcpy(t->g_fwd, &gf, sizeof gf, hipMemcpyHostToDevice);
    e = e ? e : hipMemcpy(t->g_bwd, &gb, sizeof gb, hipMemcpyHostToDevice);
    e = e ? e : hipMemcpy(t->g_eval, &ge, sizeof ge, hipMemcpyHostToDevice);
    e = e ? e : hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        ethcnn_train_destroy(t);
        return set_err(c, ETHCNN_ERR_DEVICE, "trainer setup: %s", hipGetErrorString(e));
    }
    *out = t;
    return ETHCNN_OK;
}

extern "C" void ethcnn_train_destroy(ethcnn_trainer* t) {
    if (!t) return;
    (void)hipSetDevice(t->c->device);
    (void)hipStreamSynchronize(t->c->stream);
    for (void* p : t->allocs) (void)hipFree(p);
    for (int s = 0; s < 2; ++s)
        if (t->data[s]) (void)hipFree(t->data[s]);
    delete t;
}

extern "C" const char* ethcnn_train_last_error(const ethcnn_trainer* t) { return t ? t->err.c_str() : "trainer is NULL"; }

// Box-Muller over splitmix64 draws; |x| > 2 sigma redrawn (tf.truncated_normal's rule)
static double trunc_normal(uint64_t& state) {
    for (;;) {
        state += 0x9E3779B97F4A7C15ull;
        const uint64_t a = mix64(state);
        state += 0x9E3779B97F4A7C15ull;
        const uint64_t b = mix64(state);
        const double u1 = ((double)(a >> 11) + 1.0) * (1.0 / 9007199254740992.0), u2 = (double)(b >> 11) * (1.0 / 9007199254740992.0);
        const double z = std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
        if (std::fabs(z) <= 2.0) return z;
    }
}

extern "C" int ethcnn_train_init_weights(ethcnn_trainer* t, uint64_t seed) {
    if (!t) return ETHCNN_ERR_ARG;
    std::vector<float> blob(kBlobFloats);
    for (int i = 0; i < kNumTensors; ++i) {
        const TensorDesc& d = kTensors[i];
        float* out = blob.data() + d.offset_bytes / 4;
        uint64_t state = mix64(seed ^ (0xA0761D6478BD642Full * (uint64_t)(i + 1)));
        const bool constant_bias = d.rank == 1 && t->net == ETHCNN_TRAIN_NET_AI;  // LDP: bias_variable is truncated normal too
        for (size_t k = 0; k < d.count(); ++k) out[k] = constant_bias ? 0.01f : (float)(0.1 * trunc_normal(state));
    }
    return ethcnn_train_set_blob(t, blob.data(), nullptr, kBlobFloats);
}

extern "C" int ethcnn_train_set_blob(ethcnn_trainer* t, const float* blob, const float* accum, size_t n) {
    if (!t) return ETHCNN_ERR_ARG;
    if (!blob || n != kBlobFloats) return terr(t, ETHCNN_ERR_ARG, "blob must hold %zu floats", kBlobFloats);
    hipStream_t s = t->c->stream;
    TCHK(t, hipSetDevice(t->c->device));
    TCHK(t, hipMemcpyAsync(t->W, blob, kBlobFloats * 4, hipMemcpyHostToDevice, s));
    if (accum) TCHK(t, hipMemcpyAsync(t->acc, accum, kBlobFloats * 4, hipMemcpyHostToDevice, s));
    else TCHK(t, hipMemsetAsync(t->acc, 0, kBlobFloats * 4, s));
    TCHK(t, hipStreamSynchronize(s));
    return 0;
}

extern "C" int ethcnn_train_get_blob(ethcnn_trainer* t, float* blob, float* accum, size_t n) {
    if (!t) return ETHCNN_ERR_ARG;
    if (!blob || n != kBlobFloats) return terr(t, ETHCNN_ERR_ARG, "blob must hold %zu floats", kBlobFloats);
    hipStream_t s = t->c->stream;
    TCHK(t, hipSetDevice(t->c->device));
    TCHK(t, hipMemcpyAsync(blob, t->W, kBlobFloats * 4, hipMemcpyDeviceToHost, s));
    if (accum) TCHK(t, hipMemcpyAsync(accum, t->acc, kBlobFloats * 4, hipMemcpyDeviceToHost, s));
    TCHK(t, hipStreamSynchronize(s));
    return 0;
}

// the checks every record takes on the device, then the set's bookkeeping: `p` (n records in HBM) becomes set `set`.  LDP: every record
// carries the slot QPs sq[4] (one pass on the device).  On failure `p` is left to the caller.
static int install_samples(ethcnn_trainer* t, int set, uint8_t* p, int64_t n, const int sq[4]) {
    if (t->net == ETHCNN_TRAIN_NET_LDP) {
        const int nblk = (int)std::min<int64_t>(1024, (n + 255) / 256);
        long* d_bad = nullptr;
        std::vector<long> bad((size_t)nblk);
        const uint32_t want = (uint32_t)sq[0] | (uint32_t)sq[1] << 8 | (uint32_t)sq[2] << 16 | (uint32_t)sq[3] << 24;
        hipError_t e = hipMalloc(&d_bad, sizeof(long) * nblk);
        if (e == hipSuccess) {
            launch_check_slots(t->c->stream, p, (long)n, want, d_bad, nblk);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(bad.data(), d_bad, sizeof(long) * nblk, hipMemcpyDeviceToHost, t->c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(t->c->stream);
        (void)hipFree(d_bad);
        if (e != hipSuccess) return terr(t, ETHCNN_ERR_DEVICE, "sample check: %s", hipGetErrorString(e));
        const long first = *std::min_element(bad.begin(), bad.end());
        if (first < n) {
            uint8_t r[3 * kSlotBytes + 1] = {0};
            (void)hipMemcpy(r, p + (size_t)first * kRecLdp + kSlotBase, sizeof r, hipMemcpyDeviceToHost);
            return terr(t, ETHCNN_ERR_FORMAT, "record %ld: slot QPs %d %d %d %d differ from record 0's %d %d %d %d", first, r[0],
                        r[kSlotBytes], r[2 * kSlotBytes], r[3 * kSlotBytes], sq[0], sq[1], sq[2], sq[3]);
        }
    }
    if (t->data[set]) (void)hipFree(t->data[set]);
    if (t->net == ETHCNN_TRAIN_NET_LDP) {
        for (int q = 0; q < 52; ++q) t->slot_of_qp[set][q] = -1;
        for (int q = 0; q < 4; ++q) {
            t->slot_qps[set][q] = sq[q];
            t->slot_of_qp[set][sq[q]] = q;
        }
        if (set == ETHCNN_TRAIN_SET_TRAIN) {  // the QP list defaults to the four slots (every MODEL_TYPE trains on all of them)
            std::memcpy(t->qps, sq, sizeof(int) * 4);
            t->nqps = 4;
        }
    }
    t->data[set] = p;
    t->nrec[set] = n;
    return 0;
}

extern "C" int ethcnn_train_set_samples(ethcnn_trainer* t, int set, const uint8_t* rec, size_t nbytes) {
    if (!t) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return terr(t, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    if (!rec || nbytes == 0) return terr(t, ETHCNN_ERR_ARG, "no sample records");
    const int rb = t->net == ETHCNN_TRAIN_NET_LDP ? kRecLdp : kRec;
    if (nbytes % rb) return terr(t, ETHCNN_ERR_FORMAT, "%zu bytes is not a whole number of %d-byte records", nbytes, rb);
    if (nbytes / rb > 0x7fffffffull) return terr(t, ETHCNN_ERR_ARG, "more than 2^31 - 1 records");
    int sq[4] = {0, 0, 0, 0};
    if (t->net == ETHCNN_TRAIN_NET_LDP) {  // record 0's slot QPs: four distinct values in 0..51
        for (int q = 0; q < 4; ++q) {
            sq[q] = rec[kSlotBase + kSlotBytes * q];
            if (sq[q] > 51) return terr(t, ETHCNN_ERR_FORMAT, "record 0: slot %d holds QP %d, outside 0..51", q, sq[q]);
            for (int k = 0; k < q; ++k)
                if (sq[k] == sq[q]) return terr(t, ETHCNN_ERR_FORMAT, "record 0: slots %d and %d both hold QP %d", k, q, sq[q]);
        }
    }
    TCHK(t, hipSetDevice(t->c->device));
    TCHK(t, hipStreamSynchronize(t->c->stream));
    if (t->data[set]) {
        (void)hipFree(t->data[set]);
        t->data[set] = nullptr;
        t->nrec[set] = 0;
    }
    void* p = nullptr;
    if (hipMalloc(&p, nbytes) != hipSuccess) {
        (void)hipGetLastError();
        return terr(t, ETHCNN_ERR_NOMEM, "%zu bytes of samples do not fit in device memory", nbytes);
    }
    if (hipMemcpy(p, rec, nbytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p);
        return terr(t, ETHCNN_ERR_DEVICE, "sample upload failed");
    }
    const int rc = install_samples(t, set, (uint8_t*)p, (int64_t)(nbytes / rb), sq);
    if (rc) (void)hipFree(p);
    return rc;
}

// the same from a sample set already in HBM (include/ethcnn.h "sample sets"): adopted (take) or copied device to device
extern "C" int ethcnn_train_set_samples_from(ethcnn_trainer* t, int set, ethcnn_samples* sm, int take) {
    if (!t) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return terr(t, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    if (!sm || !sm->built || sm->count == 0) return terr(t, ETHCNN_ERR_ARG, "no sample records (the sample set is not built or empty)");
    if (sm->c != t->c) return terr(t, ETHCNN_ERR_ARG, "the sample set and the trainer live on different contexts");
    if (sm->kind != t->net)
        return terr(t, ETHCNN_ERR_FORMAT, "a sample set of %d-byte records does not feed this trainer's net (%d-byte records)",
                    sm->record_bytes(), t->net == ETHCNN_TRAIN_NET_LDP ? kRecLdp : kRec);
    if (sm->count > 0x7fffffffll) return terr(t, ETHCNN_ERR_ARG, "more than 2^31 - 1 records");
    TCHK(t, hipSetDevice(t->c->device));
    TCHK(t, hipStreamSynchronize(t->c->stream));
    const size_t nbytes = (size_t)sm->count * (size_t)sm->record_bytes();
    uint8_t* p = sm->data;
    if (!take) {
        if (hipMalloc((void**)&p, nbytes) != hipSuccess) {
            (void)hipGetLastError();
            return terr(t, ETHCNN_ERR_NOMEM, "%zu bytes of samples do not fit in device memory", nbytes);
        }
        // (on the context's stream, which does not wait for the null stream: a device-to-device hipMemcpy there may still be
        // running when the check below reads its destination)
        if (hipMemcpyAsync(p, sm->data, nbytes, hipMemcpyDeviceToDevice, t->c->stream) != hipSuccess ||
            hipStreamSynchronize(t->c->stream) != hipSuccess) {
            (void)hipFree(p);
            return terr(t, ETHCNN_ERR_DEVICE, "sample copy failed");
        }
    }
    const int rc = install_samples(t, set, p, sm->count, sm->qps);
    if (rc) {
        if (!take) (void)hipFree(p);
        return rc;
    }
    if (take) {  // the trainer owns the buffer now; the set is empty (and may take sequences again)
        sm->data = nullptr;
        sm->count = 0;
        sm->seqs.clear();
        sm->built = false;
    }
    return 0;
}

extern "C" int ethcnn_train_set_qps(ethcnn_trainer* t, const int* qps, int n) {
    if (!t) return ETHCNN_ERR_ARG;
    if (!qps || n <= 0 || n > 52) return terr(t, ETHCNN_ERR_ARG, "the QP list must hold 1..52 entries");
    for (int i = 0; i < n; ++i)
        if (qps[i] < 0 || qps[i] > 51) return terr(t, ETHCNN_ERR_ARG, "QP %d outside 0..51", qps[i]);
    if (t->net == ETHCNN_TRAIN_NET_LDP) {
        if (!t->data[ETHCNN_TRAIN_SET_TRAIN]) return terr(t, ETHCNN_ERR_ARG, "LDP: upload the training samples before the QP list");
        for (int i = 0; i < n; ++i)
            if (t->slot_of_qp[ETHCNN_TRAIN_SET_TRAIN][qps[i]] < 0)
                return terr(t, ETHCNN_ERR_ARG, "QP %d is not a slot QP of the training samples", qps[i]);
    }
    std::memcpy(t->qps, qps, sizeof(int) * n);
    t->nqps = n;
    return 0;
}

extern "C" int ethcnn_train_run(ethcnn_trainer* t, int64_t first_step, int64_t nsteps) {
    if (!t) return ETHCNN_ERR_ARG;
    if (first_step < 0 || nsteps < 0) return terr(t, ETHCNN_ERR_ARG, "negative step");
    if (int rc = ready(t)) return rc;
    TCHK(t, hipSetDevice(t->c->device));
    for (int64_t i = 0; i < nsteps; ++i)
        if (int rc = enqueue_step(t, first_step + i, false)) return rc;
    return 0;
}

extern "C" int ethcnn_train_last_stats(ethcnn_trainer* t, float loss3[3], float acc3[3]) {
    if (!t) return ETHCNN_ERR_ARG;
    TCHK(t, hipSetDevice(t->c->device));
    return read_stats(t, loss3, acc3);
}

extern "C" int ethcnn_train_step_indices(ethcnn_trainer* t, int64_t step, const int32_t* idx, const int* qp, int n, float loss3[3],
                                         float acc3[3]) {
    if (!t) return ETHCNN_ERR_ARG;
    if (int rc = ready(t)) return rc;
    if (!idx || !qp || n != t->B) return terr(t, ETHCNN_ERR_ARG, "an explicit batch needs %d indices and QPs", t->B);
    if (step < 0) return terr(t, ETHCNN_ERR_ARG, "negative step");
    for (int i = 0; i < n; ++i) {
        if (idx[i] < 0 || idx[i] >= t->nrec[0]) return terr(t, ETHCNN_ERR_ARG, "sample index %d outside 0..%lld", idx[i], (long long)t->nrec[0] - 1);
        if (qp[i] < 0 || qp[i] > 51) return terr(t, ETHCNN_ERR_ARG, "QP %d outside 0..51", qp[i]);
        if (t->net == ETHCNN_TRAIN_NET_LDP && t->slot_of_qp[ETHCNN_TRAIN_SET_TRAIN][qp[i]] < 0)
            return terr(t, ETHCNN_ERR_ARG, "QP %d is not a slot QP of the training samples", qp[i]);
    }
    TCHK(t, hipSetDevice(t->c->device));
    hipStream_t s = t->c->stream;
    TCHK(t, hipMemcpyAsync(t->idx_in, idx, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    TCHK(t, hipMemcpyAsync(t->qp_in, qp, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    TCHK(t, hipStreamSynchronize(s));
    if (int rc = enqueue_step(t, step, true)) return rc;
    return read_stats(t, loss3, acc3);
}

extern "C" int ethcnn_train_evaluate(ethcnn_trainer* t, int set, const int32_t* idx, int64_t n, int qp, float loss3[3], float acc3[3],
                                     float* probs) {
    if (!t) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return terr(t, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    if (!t->data[set]) return terr(t, ETHCNN_ERR_ARG, "no samples in set %d", set);
    const bool ldp = t->net == ETHCNN_TRAIN_NET_LDP;
    if (!(qp >= 0 && qp <= 51) && !(ldp && qp == -1))
        return terr(t, ETHCNN_ERR_ARG, ldp ? "QP %d is neither a slot QP nor -1" : "QP %d outside 0..51", qp);
    if (ldp && qp >= 0 && t->slot_of_qp[set][qp] < 0) return terr(t, ETHCNN_ERR_ARG, "QP %d is not a slot QP of set %d", qp, set);
    if (n <= 0 || n > 0x7fffffffll || (!idx && n > t->nrec[set])) return terr(t, ETHCNN_ERR_ARG, "bad sample count %lld", (long long)n);
    if (idx)
        for (int64_t i = 0; i < n; ++i)
            if (idx[i] < 0 || idx[i] >= t->nrec[set]) return terr(t, ETHCNN_ERR_ARG, "sample index %d outside 0..%lld", idx[i], (long long)t->nrec[set] - 1);
    TCHK(t, hipSetDevice(t->c->device));
    hipStream_t s = t->c->stream;
    t->c->done_armed = 0;
    std::vector<int32_t> ids;
    if (!idx) {
        ids.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) ids[(size_t)i] = (int32_t)i;
        idx = ids.data();
    }
    std::vector<int32_t> mixed;  // qp == -1: sample i at the slot draw(2, 0, i, 0) picks among the four
    if (qp < 0) {
        mixed.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i)
            mixed[(size_t)i] = t->slot_qps[set][((draw(t->opt.seed, kStreamQp, 0, (uint64_t)i, 0) >> 32) * 4ull) >> 32];
    }
    float *Pn = nullptr, *Ln = nullptr;
    int32_t *In = nullptr, *Qn = nullptr;
    if (hipMalloc(&Pn, (size_t)n * kTOut * 4) != hipSuccess || hipMalloc(&Ln, (size_t)n * 16 * 4) != hipSuccess ||
        hipMalloc(&In, (size_t)n * 4) != hipSuccess || (qp < 0 && hipMalloc(&Qn, (size_t)n * 4) != hipSuccess)) {
        (void)hipGetLastError();
        (void)hipFree(Pn); (void)hipFree(Ln); (void)hipFree(In); (void)hipFree(Qn);
        return terr(t, ETHCNN_ERR_NOMEM, "cannot allocate the evaluation buffers of %lld samples", (long long)n);
    }
    hipError_t e = hipMemcpyAsync(In, idx, (size_t)n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && Qn) e = hipMemcpyAsync(Qn, mixed.data(), (size_t)n * 4, hipMemcpyHostToDevice, s);
    for (int64_t c0 = 0; e == hipSuccess && c0 < n; c0 += t->cap) {
        const int nb = (int)std::min<int64_t>(t->cap, n - c0);
        enqueue_forward(t, set, nb, In + c0, Qn ? Qn + c0 : nullptr, qp, 0, 0, Pn + c0 * kTOut, Ln + c0 * 16, t->g_eval, t->t_eval);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        float* st = t->stats;
        launch_loss(s, Pn, Ln, (int)n, st, nullptr);  // ONE batch over all n samples
        e = hipGetLastError();
    }
    if (e == hipSuccess && probs) e = hipMemcpyAsync(probs, Pn, (size_t)n * kTOut * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(Pn); (void)hipFree(Ln); (void)hipFree(In); (void)hipFree(Qn);
    if (e != hipSuccess) return terr(t, ETHCNN_ERR_DEVICE, "evaluation: %s", hipGetErrorString(e));
    return read_stats(t, loss3, acc3);
}

extern "C" int ethcnn_train_debug_fetch(ethcnn_trainer* t, int which, float* out, size_t nfloats) {
    if (!t) return ETHCNN_ERR_ARG;
    const void* src = nullptr;
    size_t need = 0;
    std::vector<int32_t> iq;
    switch (which) {
        case ETHCNN_TRAIN_DBG_GRADS: src = t->grad; need = kBlobFloats; break;
        case ETHCNN_TRAIN_DBG_ACCUM: src = t->acc; need = kBlobFloats; break;
        case ETHCNN_TRAIN_DBG_MASK_FC1: src = t->M1; need = (size_t)t->B * kTV; break;
        case ETHCNN_TRAIN_DBG_MASK_FC2: src = t->M2; need = (size_t)t->B * kT2; break;
        case ETHCNN_TRAIN_DBG_PROBS: src = t->P; need = (size_t)t->B * kTOut; break;
        case ETHCNN_TRAIN_DBG_INDICES: need = (size_t)t->B * 2; break;
        case ETHCNN_TRAIN_DBG_H1: src = t->A1; need = (size_t)t->B * kTV; break;
        default: return terr(t, ETHCNN_ERR_ARG, "unknown debug buffer %d", which);
    }
    if (!out || nfloats != need) return terr(t, ETHCNN_ERR_ARG, "debug buffer %d holds %zu floats", which, need);
    TCHK(t, hipSetDevice(t->c->device));
    hipStream_t s = t->c->stream;
    if (which == ETHCNN_TRAIN_DBG_INDICES) {
        iq.resize((size_t)t->B * 2);
        TCHK(t, hipMemcpyAsync(iq.data(), t->idx, sizeof(int32_t) * t->B, hipMemcpyDeviceToHost, s));
        TCHK(t, hipMemcpyAsync(iq.data() + t->B, t->qp, sizeof(int32_t) * t->B, hipMemcpyDeviceToHost, s));
        TCHK(t, hipStreamSynchronize(s));
        for (int b = 0; b < t->B; ++b) {
            out[2 * b] = (float)iq[b];
            out[2 * b + 1] = (float)iq[t->B + b];
        }
        return 0;
    }
    TCHK(t, hipMemcpyAsync(out, src, need * 4, hipMemcpyDeviceToHost, s));
    TCHK(t, hipStreamSynchronize(s));
    return 0;
}
