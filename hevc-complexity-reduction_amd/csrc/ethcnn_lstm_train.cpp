// ethcnn_lstm_train.cpp -- an ETH-LSTM trainer's state (include/ethcnn.h "ETH-LSTM training"): options, weight / accumulator /
// gradient blobs, workspaces, the GEMM descriptors over them, the QP list, and the entry points that touch nothing else.  Everything
// that enqueues a step, and the sample sets, are the engine's (ethcnn_lstm_train_group.cpp); the solo entry points at the end of this
// file hand over to the trainer's own engine of K = 1.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ethcnn_ctx.h"
#include "ethcnn_lstm_train.h"
#include "ethcnn_lstm_train_host.h"

using namespace ethcnn::lstm_train;
using ethcnn::train::add_desc;
using ethcnn::kLstmBlobFloats;
using ethcnn::kLstmTensors;
using ethcnn::kNumLstmTensors;
using ethcnn::TensorDesc;
using ethcnn::train::GemmDesc;
using ethcnn::train::GemmGroup;

namespace {
constexpr int kEvalChunk = 256;  // samples per evaluation piece (5120 rows)
const int kH[3] = {64, 128, 256}, kHOff[3] = {0, 64, 192}, kC2[3] = {48, 96, 192}, kC2Off[3] = {0, 48, 144};
const int kC3[3] = {1, 4, 16}, kC3Off[3] = {0, 1, 5}, kH1Off[3] = {0, 70, 204}, kH2Off[3] = {0, 54, 156};
const char* kCellTag[3] = {"64", "32", "16"};

int lstm_tensor_off(const std::string& name) {
    for (int t = 0; t < kNumLstmTensors; ++t)
        if (name == kLstmTensors[t].name) return (int)(kLstmTensors[t].offset_bytes / 4);
    return -1;
}
}  // namespace

template <typename T>
static int talloc(ethcnn_lstm_trainer* t, T** p, size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 4) != hipSuccess) {
        (void)hipGetLastError();
        return terr(t, ETHCNN_ERR_NOMEM, "cannot allocate %zu bytes of device memory", count * sizeof(T));
    }
    t->allocs.push_back(q);
    *p = (T*)q;
    return 0;
}

// input projections of `rows` rows: Z_cell = X[:, cell columns] x kernel[0:H, :]
GemmGroup lstm_proj_group(const ethcnn_lstm_trainer* t, int rows) {
    GemmGroup g{};
    for (int c = 0; c < 3; ++c) {
        GemmDesc d{};
        d.M = rows; d.N = 4 * kH[c]; d.K = kH[c];
        d.A = t->u.X + kHOff[c]; d.sam = kVec; d.sak = 1;
        d.B[0] = t->W + t->o.kern[c]; d.sbk[0] = 4 * kH[c]; d.sbn[0] = 1;
        d.C = t->u.Z[c]; d.ldc = 4 * kH[c];
        add_desc(g, d);
    }
    return g;
}

// the 18 tensors' gradients, K = rows, written into grad at their blob offsets
GemmGroup lstm_grad_group(const ethcnn_lstm_trainer* t, int rows) {
    GemmGroup g{};
    for (int c = 0; c < 3; ++c) {
        const int H = kH[c];
        GemmDesc x{};  // kernel rows 0 .. H - 1: x^T dZ
        x.M = H; x.N = 4 * H; x.K = rows;
        x.A = t->u.X + kHOff[c]; x.sam = 1; x.sak = kVec;
        x.B[0] = t->u.dZ[c]; x.sbk[0] = 4 * H; x.sbn[0] = 1;
        x.C = t->grad + t->o.kern[c]; x.ldc = 4 * H;
        add_desc(g, x);
        GemmDesc h{};  // kernel rows H .. 2H - 1 and the bias (ones column): [h_prev | 1]^T dZ
        h.M = H + 1; h.N = 4 * H; h.K = rows; h.msplit = H;
        h.A = t->u.HP[c]; h.sam = 1; h.sak = H + 1;
        h.B[0] = t->u.dZ[c]; h.sbk[0] = 4 * H; h.sbn[0] = 1;
        h.C = t->grad + t->o.kern[c] + (long)H * 4 * H; h.C2 = t->grad + t->o.bias[c]; h.ldc = 4 * H;
        add_desc(g, h);
        GemmDesc e{};  // fc2: [h (dropped) | ef | 1]^T dZ2
        e.M = H + kEf + 1; e.N = kC2[c]; e.K = rows; e.msplit = H + kEf;
        e.A = t->u.H1 + kH1Off[c]; e.sam = 1; e.sak = kLdH1;
        e.B[0] = t->u.dZ2 + kC2Off[c]; e.sbk[0] = kFc2; e.sbn[0] = 1;
        e.C = t->grad + t->o.w2[c]; e.C2 = t->grad + t->o.b2[c]; e.ldc = kC2[c];
        add_desc(g, e);
        GemmDesc y{};  // fc3: [h2 (dropped) | ef | 1]^T dZ3
        y.M = kC2[c] + kEf + 1; y.N = kC3[c]; y.K = rows; y.msplit = kC2[c] + kEf;
        y.A = t->u.H2 + kH2Off[c]; y.sam = 1; y.sak = kLdH2;
        y.B[0] = t->u.dZ3 + kC3Off[c]; y.sbk[0] = kOut; y.sbn[0] = 1;
        y.C = t->grad + t->o.w3[c]; y.C2 = t->grad + t->o.b3[c]; y.ldc = kC3[c];
        add_desc(g, y);
    }
    return g;
}

int lstm_member_create(ethcnn_ctx* c, const ethcnn_lstm_train_options* opt, ethcnn_lstm_trainer** out) {
    *out = nullptr;
    if (opt->batch <= 0 || opt->batch > 4096) return set_err(c, ETHCNN_ERR_ARG, "batch must be in 1..4096, got %d", opt->batch);
    if (opt->decay_steps <= 0) return set_err(c, ETHCNN_ERR_ARG, "decay_steps must be positive");
    if (!std::isfinite(opt->lr_init) || !std::isfinite(opt->momentum) || !std::isfinite(opt->decay_rate))
        return set_err(c, ETHCNN_ERR_ARG, "non-finite optimiser option");
    if (!std::isfinite(opt->qp_scale) || opt->qp_scale < 0.f) return set_err(c, ETHCNN_ERR_ARG, "qp_scale must be finite and >= 0 (0 means 1.0)");
    if (!std::isfinite(opt->clip_norm) || opt->clip_norm < 0.f) return set_err(c, ETHCNN_ERR_ARG, "clip_norm must be finite and >= 0 (0 means no clip)");
    if (hipSetDevice(c->device) != hipSuccess) return set_err(c, ETHCNN_ERR_DEVICE, "hipSetDevice(%d) failed", c->device);
    ethcnn_lstm_trainer* t = new (std::nothrow) ethcnn_lstm_trainer;
    if (!t) return set_err(c, ETHCNN_ERR_NOMEM, "out of memory");
    t->c = c;
    t->opt = *opt;
    t->B = opt->batch;
    t->cap = std::max(t->B, kEvalChunk);
    t->qp_scale = opt->qp_scale == 0.f ? 1.f : opt->qp_scale;
    for (int k = 0; k < 3; ++k) {
        const std::string pre = std::string("RNN") + kCellTag[k] + "/";
        t->o.kern[k] = lstm_tensor_off(pre + "multi_rnn_cell/cell_0/lstm_cell/kernel");
        t->o.bias[k] = lstm_tensor_off(pre + "multi_rnn_cell/cell_0/lstm_cell/bias");
        t->o.w2[k] = lstm_tensor_off(pre + "fc2/full_connect_w");
        t->o.b2[k] = lstm_tensor_off(pre + "fc2/full_connect_b");
        t->o.w3[k] = lstm_tensor_off(pre + "fc3/full_connect_w");
        t->o.b3[k] = lstm_tensor_off(pre + "fc3/full_connect_b");
    }
    const size_t R = (size_t)t->cap * kSteps;
    LstmBufs& u = t->u;
    int rc = 0;
    rc = rc ? rc : talloc(t, &t->W, kLstmBlobFloats);
    rc = rc ? rc : talloc(t, &t->acc, kLstmBlobFloats);
    rc = rc ? rc : talloc(t, &t->grad, kLstmBlobFloats);
    rc = rc ? rc : talloc(t, &t->stats, 8);
    rc = rc ? rc : talloc(t, &t->part, kNormBlocks);
    rc = rc ? rc : talloc(t, &t->idx, (size_t)t->cap);
    rc = rc ? rc : talloc(t, &t->idx_in, (size_t)t->cap);
    rc = rc ? rc : talloc(t, &u.X, R * kVec);
    rc = rc ? rc : talloc(t, &u.lab, R * 16);
    rc = rc ? rc : talloc(t, &u.E, R * kEf);
    for (int k = 0; k < 3; ++k) {
        rc = rc ? rc : talloc(t, &u.Z[k], R * 4 * kH[k]);
        rc = rc ? rc : talloc(t, &u.dZ[k], R * 4 * kH[k]);
        rc = rc ? rc : talloc(t, &u.HP[k], R * (kH[k] + 1));
    }
    rc = rc ? rc : talloc(t, &u.Cpre, R * kVec);
    rc = rc ? rc : talloc(t, &u.C, R * kVec);
    rc = rc ? rc : talloc(t, &u.Hout, R * kVec);
    rc = rc ? rc : talloc(t, &u.M1, R * kVec);
    rc = rc ? rc : talloc(t, &u.H1, R * kLdH1);
    rc = rc ? rc : talloc(t, &u.A2, R * kFc2);
    rc = rc ? rc : talloc(t, &u.M2, R * kFc2);
    rc = rc ? rc : talloc(t, &u.H2, R * kLdH2);
    rc = rc ? rc : talloc(t, &u.P, R * kOut);
    rc = rc ? rc : talloc(t, &u.dZ3, R * kOut);
    rc = rc ? rc : talloc(t, &u.dZ2, R * kFc2);
    rc = rc ? rc : talloc(t, &u.dH, R * kVec);
    if (rc) {
        const std::string why = t->err;
        lstm_member_destroy(t);
        return set_err(c, rc, "%s", why.c_str());
    }
    // zeroed once: rows past a short evaluation piece are computed by the projection GEMM but never read
    hipError_t e = hipSuccess;
    for (void* p : {(void*)t->W, (void*)t->acc, (void*)t->grad}) e = e ? e : hipMemsetAsync(p, 0, kLstmBlobFloats * 4, c->stream);
    e = e ? e : hipMemsetAsync(u.X, 0, R * kVec * 4, c->stream);
    e = e ? e : hipMemsetAsync(t->stats, 0, 32, c->stream);
    e = e ? e : hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        lstm_member_destroy(t);
        return set_err(c, ETHCNN_ERR_DEVICE, "LSTM trainer setup: %s", hipGetErrorString(e));
    }
    *out = t;
    return ETHCNN_OK;
}

void lstm_member_destroy(ethcnn_lstm_trainer* t) {
    (void)hipSetDevice(t->c->device);
    (void)hipStreamSynchronize(t->c->stream);
    for (void* p : t->allocs) (void)hipFree(p);
    delete t;
}

extern "C" const char* ethcnn_lstm_train_last_error(const ethcnn_lstm_trainer* t) { return t ? t->err.c_str() : "trainer is NULL"; }

extern "C" int ethcnn_lstm_train_init_weights(ethcnn_lstm_trainer* t, uint64_t seed) {
    if (!t) return ETHCNN_ERR_ARG;
    std::vector<float> blob(kLstmBlobFloats);
    for (int i = 0; i < kNumLstmTensors; ++i) {
        const TensorDesc& d = kLstmTensors[i];
        float* out = blob.data() + d.offset_bytes / 4;
        // tf.get_variable without an initializer: glorot_uniform, limit sqrt(6 / (fan_in + fan_out)); a 1-D [n] variable has
        // fan_in = fan_out = n.  LSTMCell's bias: zeros.
        double limit;
        if (d.rank == 2) limit = std::sqrt(6.0 / (double)(d.shape[0] + d.shape[1]));
        else if (std::strstr(d.name, "full_connect_b")) limit = std::sqrt(3.0 / (double)d.shape[0]);
        else limit = 0.0;
        for (size_t k = 0; k < d.count(); ++k) {
            const double uu = (double)(draw(seed, kStreamLstmInit, (uint64_t)i, 0, (uint64_t)k) >> 11) * (1.0 / 9007199254740992.0);
            out[k] = (float)((2.0 * uu - 1.0) * limit);
        }
    }
    return ethcnn_lstm_train_set_blob(t, blob.data(), nullptr, kLstmBlobFloats);
}

extern "C" int ethcnn_lstm_train_set_blob(ethcnn_lstm_trainer* t, const float* blob, const float* accum, size_t n) {
    if (!t) return ETHCNN_ERR_ARG;
    if (!blob || n != kLstmBlobFloats) return terr(t, ETHCNN_ERR_ARG, "blob must hold %zu floats", kLstmBlobFloats);
    hipStream_t s = t->c->stream;
    TCHK(t, hipSetDevice(t->c->device));
    TCHK(t, hipMemcpyAsync(t->W, blob, kLstmBlobFloats * 4, hipMemcpyHostToDevice, s));
    if (accum) TCHK(t, hipMemcpyAsync(t->acc, accum, kLstmBlobFloats * 4, hipMemcpyHostToDevice, s));
    else TCHK(t, hipMemsetAsync(t->acc, 0, kLstmBlobFloats * 4, s));
    TCHK(t, hipStreamSynchronize(s));
    return 0;
}

extern "C" int ethcnn_lstm_train_get_blob(ethcnn_lstm_trainer* t, float* blob, float* accum, size_t n) {
    if (!t) return ETHCNN_ERR_ARG;
    if (!blob || n != kLstmBlobFloats) return terr(t, ETHCNN_ERR_ARG, "blob must hold %zu floats", kLstmBlobFloats);
    hipStream_t s = t->c->stream;
    TCHK(t, hipSetDevice(t->c->device));
    TCHK(t, hipMemcpyAsync(blob, t->W, kLstmBlobFloats * 4, hipMemcpyDeviceToHost, s));
    if (accum) TCHK(t, hipMemcpyAsync(accum, t->acc, kLstmBlobFloats * 4, hipMemcpyDeviceToHost, s));
    TCHK(t, hipStreamSynchronize(s));
    return 0;
}

extern "C" int ethcnn_lstm_train_set_qps(ethcnn_lstm_trainer* t, const int* qps, int n) {
    if (!t) return ETHCNN_ERR_ARG;
    if (n < 0 || n > 52 || (n > 0 && !qps)) return terr(t, ETHCNN_ERR_ARG, "the QP list must hold 0..52 entries");
    for (int i = 0; i < n; ++i)
        if (qps[i] < 0 || qps[i] > 51) return terr(t, ETHCNN_ERR_ARG, "QP %d outside 0..51", qps[i]);
    if (n) std::memcpy(t->qps, qps, sizeof(int) * n);
    t->nqps = n;
    return 0;
}

extern "C" int64_t ethcnn_lstm_train_debug_rows(const ethcnn_lstm_trainer* t) { return t ? t->last_rows : -1; }

// ---- the solo trainer: an engine of K = 1 over the trainer itself; its messages are the trainer's
static int from_engine(ethcnn_lstm_trainer* t, int rc) {
    if (rc) t->err = t->eng->err;
    return rc;
}

extern "C" int ethcnn_lstm_train_create(ethcnn_ctx* c, const ethcnn_lstm_train_options* opt, ethcnn_lstm_trainer** out) {
    if (!c || !opt || !out) return ETHCNN_ERR_ARG;
    ethcnn_lstm_trainer* t = nullptr;
    if (int rc = lstm_member_create(c, opt, &t)) return rc;
    if (int rc = lstm_engine_create(c, {t}, false, &t->eng)) {
        lstm_member_destroy(t);
        return rc;
    }
    t->solo = true;
    *out = t;
    return ETHCNN_OK;
}

extern "C" void ethcnn_lstm_train_destroy(ethcnn_lstm_trainer* t) {
    if (!t) return;
    (void)hipSetDevice(t->c->device);
    (void)hipStreamSynchronize(t->c->stream);
    if (t->solo) lstm_engine_destroy(t->eng);
    lstm_member_destroy(t);
}

extern "C" int ethcnn_lstm_train_set_samples(ethcnn_lstm_trainer* t, int set, const uint8_t* rec, size_t nbytes) {
    return t ? from_engine(t, ethcnn_lstm_train_group_set_samples(t->eng, set, rec, nbytes)) : ETHCNN_ERR_ARG;
}

extern "C" int ethcnn_lstm_train_set_samples_from(ethcnn_lstm_trainer* t, int set, ethcnn_lstm_samples* sm, int take) {
    return t ? from_engine(t, ethcnn_lstm_train_group_set_samples_from(t->eng, set, sm, take)) : ETHCNN_ERR_ARG;
}

extern "C" int64_t ethcnn_lstm_train_num_samples(const ethcnn_lstm_trainer* t, int set) {
    return t ? ethcnn_lstm_train_group_num_samples(t->eng, 0, set) : -1;
}

extern "C" int ethcnn_lstm_train_run(ethcnn_lstm_trainer* t, int64_t first_step, int64_t nsteps) {
    return t ? from_engine(t, ethcnn_lstm_train_group_run(t->eng, first_step, nsteps)) : ETHCNN_ERR_ARG;
}

extern "C" int ethcnn_lstm_train_last_stats(ethcnn_lstm_trainer* t, float loss3[3], float acc3[3]) {
    return t ? from_engine(t, ethcnn_lstm_train_group_last_stats(t->eng, loss3, acc3)) : ETHCNN_ERR_ARG;
}

extern "C" int ethcnn_lstm_train_step_indices(ethcnn_lstm_trainer* t, int64_t step, const int32_t* idx, int n, float loss3[3],
                                              float acc3[3]) {
    return t ? from_engine(t, ethcnn_lstm_train_group_step_indices(t->eng, step, idx, n, loss3, acc3)) : ETHCNN_ERR_ARG;
}

extern "C" int ethcnn_lstm_train_evaluate(ethcnn_lstm_trainer* t, int set, const int32_t* idx, int64_t n, float loss3[3], float acc3[3],
                                          float* probs) {
    return t ? from_engine(t, ethcnn_lstm_train_group_evaluate(t->eng, set, idx, n, loss3, acc3, probs)) : ETHCNN_ERR_ARG;
}

extern "C" int ethcnn_lstm_train_debug_fetch(ethcnn_lstm_trainer* t, int which, float* out, size_t nfloats) {
    if (!t) return ETHCNN_ERR_ARG;
    const size_t R = (size_t)t->last_rows;
    const void* src = nullptr;
    size_t need = 0;
    switch (which) {
        case ETHCNN_LSTM_DBG_GRADS: src = t->grad; need = kLstmBlobFloats; break;
        case ETHCNN_LSTM_DBG_NORM: src = t->stats + 7; need = 1; break;
        case ETHCNN_LSTM_DBG_ACCUM: src = t->acc; need = kLstmBlobFloats; break;
        case ETHCNN_LSTM_DBG_MASK_H: src = t->u.M1; need = R * kVec; break;
        case ETHCNN_LSTM_DBG_MASK_FC2: src = t->u.M2; need = R * kFc2; break;
        case ETHCNN_LSTM_DBG_PROBS: src = t->u.P; need = (size_t)t->B * kSteps * kOut; break;
        case ETHCNN_LSTM_DBG_INDICES: need = R / kSteps; break;
        case ETHCNN_LSTM_DBG_STATE_C: src = t->u.C; need = R * kVec; break;
        case ETHCNN_LSTM_DBG_STATE_H: src = t->u.Hout; need = R * kVec; break;
        default: return terr(t, ETHCNN_ERR_ARG, "unknown debug buffer %d", which);
    }
    if (!out || nfloats != need || need == 0) return terr(t, ETHCNN_ERR_ARG, "debug buffer %d holds %zu floats", which, need);
    TCHK(t, hipSetDevice(t->c->device));
    hipStream_t s = t->c->stream;
    if (which == ETHCNN_LSTM_DBG_INDICES) {
        std::vector<int32_t> iq(need);
        TCHK(t, hipMemcpyAsync(iq.data(), t->idx, sizeof(int32_t) * need, hipMemcpyDeviceToHost, s));
        TCHK(t, hipStreamSynchronize(s));
        for (size_t b = 0; b < need; ++b) out[b] = (float)iq[b];
        return 0;
    }
    TCHK(t, hipMemcpyAsync(out, src, need * 4, hipMemcpyDeviceToHost, s));
    TCHK(t, hipStreamSynchronize(s));
    return 0;
}
