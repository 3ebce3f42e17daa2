// ethcnn_train.cpp -- a trainer's state (include/ethcnn.h "training"): options, weight / accumulator / gradient blobs, workspaces, the
// GEMM descriptors over them, the QP list, and the entry points that touch nothing else.  Everything that enqueues a step is the
// engine's (ethcnn_train_group.cpp); the solo entry points at the end of this file hand over to the trainer's own engine of K = 1.
#include <algorithm>
#include <cmath>
#include <new>
#include <cstring>
#include <string>
#include <vector>

#include "ethcnn_ctx.h"
#include "ethcnn_train.h"
#include "ethcnn_train_host.h"

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

int train_member_create(ethcnn_ctx* c, const ethcnn_train_options* opt, ethcnn_trainer** out) {
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
    if (rc) {
        const std::string why = t->err;
        train_member_destroy(t);
        return set_err(c, rc, "%s", why.c_str());
    }
    // zeroed once: rows past a short evaluation chunk are computed by the FC1 GEMM but never read
    hipError_t e = hipSuccess;
    for (void* p : {(void*)t->W, (void*)t->acc, (void*)t->grad}) e = e ? e : hipMemsetAsync(p, 0, kBlobFloats * 4, c->stream);
    e = e ? e : hipMemsetAsync(t->F, 0, R * kLdF * 4, c->stream);
    e = e ? e : hipMemsetAsync(t->stats, 0, 32, c->stream);
    e = e ? e : hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        train_member_destroy(t);
        return set_err(c, ETHCNN_ERR_DEVICE, "trainer setup: %s", hipGetErrorString(e));
    }
    *out = t;
    return ETHCNN_OK;
}

void train_member_destroy(ethcnn_trainer* t) {
    (void)hipSetDevice(t->c->device);
    (void)hipStreamSynchronize(t->c->stream);
    for (void* p : t->allocs) (void)hipFree(p);
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

// the QP list is part of the engine's member table: it takes effect with the next step, whoever enqueues it
extern "C" int ethcnn_train_set_qps(ethcnn_trainer* t, const int* qps, int n) {
    if (!t) return ETHCNN_ERR_ARG;
    if (!qps || n <= 0 || n > 52) return terr(t, ETHCNN_ERR_ARG, "the QP list must hold 1..52 entries");
    for (int i = 0; i < n; ++i)
        if (qps[i] < 0 || qps[i] > 51) return terr(t, ETHCNN_ERR_ARG, "QP %d outside 0..51", qps[i]);
    if (t->net == ETHCNN_TRAIN_NET_LDP) {
        if (!t->eng->data[ETHCNN_TRAIN_SET_TRAIN]) return terr(t, ETHCNN_ERR_ARG, "LDP: upload the training samples before the QP list");
        for (int i = 0; i < n; ++i)
            if (t->eng->slot_of_qp[ETHCNN_TRAIN_SET_TRAIN][qps[i]] < 0)
                return terr(t, ETHCNN_ERR_ARG, "QP %d is not a slot QP of the training samples", qps[i]);
    }
    std::memcpy(t->qps, qps, sizeof(int) * n);
    t->nqps = n;
    t->eng->stale = true;
    return 0;
}

// ---- the solo trainer: an engine of K = 1 over the trainer itself; its messages are the trainer's
static int from_engine(ethcnn_trainer* t, int rc) {
    if (rc) t->err = t->eng->err;
    return rc;
}

extern "C" int ethcnn_train_create(ethcnn_ctx* c, const ethcnn_train_options* opt, ethcnn_trainer** out) {
    if (!c || !opt || !out) return ETHCNN_ERR_ARG;
    ethcnn_trainer* t = nullptr;
    if (int rc = train_member_create(c, opt, &t)) return rc;
    if (int rc = train_engine_create(c, {t}, false, &t->eng)) {
        train_member_destroy(t);
        return rc;
    }
    t->solo = true;
    *out = t;
    return ETHCNN_OK;
}

extern "C" void ethcnn_train_destroy(ethcnn_trainer* t) {
    if (!t) return;
    (void)hipSetDevice(t->c->device);
    (void)hipStreamSynchronize(t->c->stream);
    if (t->solo) train_engine_destroy(t->eng);
    train_member_destroy(t);
}

extern "C" int ethcnn_train_set_samples(ethcnn_trainer* t, int set, const uint8_t* rec, size_t nbytes) {
    return t ? from_engine(t, ethcnn_train_group_set_samples(t->eng, set, rec, nbytes)) : ETHCNN_ERR_ARG;
}

extern "C" int ethcnn_train_set_samples_from(ethcnn_trainer* t, int set, ethcnn_samples* sm, int take) {
    return t ? from_engine(t, ethcnn_train_group_set_samples_from(t->eng, set, sm, take)) : ETHCNN_ERR_ARG;
}

extern "C" int ethcnn_train_run(ethcnn_trainer* t, int64_t first_step, int64_t nsteps) {
    return t ? from_engine(t, ethcnn_train_group_run(t->eng, first_step, nsteps)) : ETHCNN_ERR_ARG;
}

extern "C" int ethcnn_train_last_stats(ethcnn_trainer* t, float loss3[3], float acc3[3]) {
    return t ? from_engine(t, ethcnn_train_group_last_stats(t->eng, loss3, acc3)) : ETHCNN_ERR_ARG;
}

extern "C" int ethcnn_train_step_indices(ethcnn_trainer* t, int64_t step, const int32_t* idx, const int* qp, int n, float loss3[3],
                                         float acc3[3]) {
    return t ? from_engine(t, ethcnn_train_group_step_indices(t->eng, step, idx, qp, n, loss3, acc3)) : ETHCNN_ERR_ARG;
}

extern "C" int ethcnn_train_evaluate(ethcnn_trainer* t, int set, const int32_t* idx, int64_t n, int qp, float loss3[3], float acc3[3],
                                     float* probs) {
    return t ? from_engine(t, ethcnn_train_group_evaluate(t->eng, set, idx, n, &qp, loss3, acc3, probs)) : ETHCNN_ERR_ARG;
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
