// ethcnn_lstm_train.cpp -- host side of the ETH-LSTM trainer (include/ethcnn.h "ETH-LSTM training"): buffers, the GEMM descriptor
// tables, the step and evaluation sequences (kernels: ethcnn_lstm_train_kernels.hip, launch order: ethcnn_lstm_train.h).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ethcnn_ctx.h"
#include "ethcnn_lstm_samples.h"
#include "ethcnn_lstm_train.h"
#include "ethcnn_lstm_train_host.h"

using namespace ethcnn::lstm_train;
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

static int terr(ethcnn_lstm_trainer* t, int code, const char* fmt, ...) {
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

static void add_desc(GemmGroup& g, GemmDesc d) {
    d.tiles_n = (d.N + 63) / 64;
    d.tile_begin = g.tiles;
    g.tiles += ((d.M + 63) / 64) * d.tiles_n;
    d.nseg = 1;
    d.kseg[0] = 0;
    if (d.msplit == 0) d.msplit = d.M;
    g.d[g.n++] = d;
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

float lstm_lr_at(const ethcnn_lstm_trainer* t, int64_t step) {  // tf.train.exponential_decay(..., staircase=True)
    const double p = std::floor((double)step / (double)t->opt.decay_steps);
    return (float)((double)t->opt.lr_init * std::pow((double)t->opt.decay_rate, p));
}

// gather .. heads forward of nb samples; P / lab: where this piece's probabilities and labels go
static void enqueue_forward(ethcnn_lstm_trainer* t, int set, int nb, const int32_t* d_idx, uint64_t step, int dropout, float* P,
                            float* lab, const GemmGroup* grp, int tiles) {
    hipStream_t s = t->c->stream;
    GatherArgs a{};
    a.data = t->data[set];
    a.nrec = t->nrec[set];
    a.idx_in = d_idx;
    a.idx_out = t->idx;
    a.seed = t->opt.seed;
    a.step = step;
    a.qp_scale = t->qp_scale;
    LstmBufs u = t->u;
    u.P = P;
    u.lab = lab;
    launch_gather(s, nb, a, u);
    ethcnn::train::launch_gemm(s, grp, tiles);
    launch_fwd(s, nb, u, t->W, t->o);
    launch_heads_fwd(s, nb, u, t->W, t->o, t->opt.seed, step, dropout);
    t->last_rows = nb * kSteps;
}

static int enqueue_step(ethcnn_lstm_trainer* t, int64_t step, bool explicit_batch) {
    hipStream_t s = t->c->stream;
    t->c->done_armed = 0;  // the context's completion word does not cover these launches
    const int dropout = t->opt.dropout ? 1 : 0;
    enqueue_forward(t, ETHCNN_TRAIN_SET_TRAIN, t->B, explicit_batch ? t->idx_in : nullptr, (uint64_t)step, dropout, t->u.P, t->u.lab,
                    t->g_fwd, t->t_fwd);
    ethcnn::train::launch_loss(s, t->u.P, t->u.lab, t->B * kSteps, t->stats, t->u.dZ3);
    launch_heads_bwd(s, t->B, t->u, t->W, t->o, dropout);
    launch_bwd(s, t->B, t->u, t->W, t->o);
    ethcnn::train::launch_gemm(s, t->g_bwd, t->t_bwd);
    launch_norm_update(s, t->W, t->acc, t->grad, t->part, t->opt.clip_norm, lstm_lr_at(t, step), t->opt.momentum, (long)kLstmBlobFloats,
                       t->stats);
    TCHK(t, hipGetLastError());
    return 0;
}

static int read_stats(ethcnn_lstm_trainer* t, float* loss3, float* acc3) {
    float st[8];
    TCHK(t, hipMemcpyAsync(st, t->stats, sizeof st, hipMemcpyDeviceToHost, t->c->stream));
    TCHK(t, hipStreamSynchronize(t->c->stream));
    for (int i = 0; i < 3; ++i) {
        if (loss3) loss3[i] = st[i];
        if (acc3) acc3[i] = st[3 + i];
    }
    return 0;
}

extern "C" int ethcnn_lstm_train_create(ethcnn_ctx* c, const ethcnn_lstm_train_options* opt, ethcnn_lstm_trainer** out) {
    if (!c || !opt || !out) return ETHCNN_ERR_ARG;
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
    rc = rc ? rc : talloc(t, &t->g_fwd, 1);
    rc = rc ? rc : talloc(t, &t->g_bwd, 1);
    rc = rc ? rc : talloc(t, &t->g_eval, 1);
    if (rc) {
        const std::string why = t->err;
        ethcnn_lstm_train_destroy(t);
        return set_err(c, rc, "%s", why.c_str());
    }
    // zeroed once: rows past a short evaluation piece are computed by the projection GEMM but never read
    hipError_t e = hipSuccess;
    for (void* p : {(void*)t->W, (void*)t->acc, (void*)t->grad}) e = e ? e : hipMemsetAsync(p, 0, kLstmBlobFloats * 4, c->stream);
    e = e ? e : hipMemsetAsync(u.X, 0, R * kVec * 4, c->stream);
    e = e ? e : hipMemsetAsync(t->stats, 0, 32, c->stream);
    const GemmGroup gf = lstm_proj_group(t, t->B * kSteps), gb = lstm_grad_group(t, t->B * kSteps), ge = lstm_proj_group(t, t->cap * kSteps);
    t->t_fwd = gf.tiles; t->t_bwd = gb.tiles; t->t_eval = ge.tiles;
    e = e ? e : hipMemcpy(t->g_fwd, &gf, sizeof gf, hipMemcpyHostToDevice);
    e = e ? e : hipMemcpy(t->g_bwd, &gb, sizeof gb, hipMemcpyHostToDevice);
    e = e ? e : hipMemcpy(t->g_eval, &ge, sizeof ge, hipMemcpyHostToDevice);
    e = e ? e : hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        ethcnn_lstm_train_destroy(t);
        return set_err(c, ETHCNN_ERR_DEVICE, "LSTM trainer setup: %s", hipGetErrorString(e));
    }
    *out = t;
    return ETHCNN_OK;
}

extern "C" void ethcnn_lstm_train_destroy(ethcnn_lstm_trainer* t) {
    if (!t) return;
    (void)hipSetDevice(t->c->device);
    (void)hipStreamSynchronize(t->c->stream);
    for (void* p : t->allocs) (void)hipFree(p);
    for (int s = 0; s < 2; ++s)
        if (t->data[s]) (void)hipFree(t->data[s]);
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

// the pass every kept sample takes on the device (k_lstm_check): *first = the first sample that fails it, n when none does
static hipError_t first_bad_sample(ethcnn_lstm_trainer* t, const uint8_t* p, size_t n, long* first) {
    const int nblk = (int)std::min<size_t>(1024, n);
    long* d_bad = nullptr;
    std::vector<long> bad((size_t)nblk);
    hipError_t e = hipMalloc(&d_bad, sizeof(long) * nblk);
    if (e == hipSuccess) {
        launch_check(t->c->stream, p, (long)n, d_bad, nblk);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(bad.data(), d_bad, sizeof(long) * nblk, hipMemcpyDeviceToHost, t->c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->c->stream);
    (void)hipFree(d_bad);
    if (e == hipSuccess) *first = *std::min_element(bad.begin(), bad.end());
    return e;
}

extern "C" int ethcnn_lstm_train_set_samples(ethcnn_lstm_trainer* t, int set, const uint8_t* rec, size_t nbytes) {
    if (!t) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return terr(t, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    if (!rec || nbytes == 0) return terr(t, ETHCNN_ERR_ARG, "no sample records");
    if (nbytes % kRecBytes) return terr(t, ETHCNN_ERR_FORMAT, "%zu bytes is not a whole number of %d-byte samples", nbytes, kRecBytes);
    const size_t nall = nbytes / kRecBytes;
    // SELECT_QP_LIST (input_data.py:126-134): keep the samples whose qps[0] is in the list
    std::vector<size_t> keep;
    keep.reserve(nall);
    for (size_t i = 0; i < nall; ++i) {
        bool on = t->nqps == 0;
        float q;
        std::memcpy(&q, rec + i * kRecBytes + 64, 4);
        for (int k = 0; k < t->nqps && !on; ++k) on = q == (float)t->qps[k];
        if (on) keep.push_back(i);
    }
    if (keep.empty()) return terr(t, ETHCNN_ERR_FORMAT, "none of the %zu samples has a selected QP", nall);
    if (keep.size() > 0x7fffffffull / kSteps) return terr(t, ETHCNN_ERR_ARG, "too many samples");
    TCHK(t, hipSetDevice(t->c->device));
    TCHK(t, hipStreamSynchronize(t->c->stream));
    const size_t n = keep.size();
    void* p = nullptr;
    if (hipMalloc(&p, n * kRecBytes) != hipSuccess) {
        (void)hipGetLastError();
        return terr(t, ETHCNN_ERR_NOMEM, "%zu bytes of samples do not fit in device memory", n * kRecBytes);
    }
    hipError_t e = hipSuccess;
    for (size_t j = 0; j < n && e == hipSuccess;) {  // runs of consecutive kept samples, one copy each
        size_t k = j + 1;
        while (k < n && keep[k] == keep[k - 1] + 1) ++k;
        e = hipMemcpy((uint8_t*)p + j * kRecBytes, rec + keep[j] * kRecBytes, (k - j) * kRecBytes, hipMemcpyHostToDevice);
        j = k;
    }
    long first = 0;
    if (e == hipSuccess) e = first_bad_sample(t, (const uint8_t*)p, n, &first);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return terr(t, ETHCNN_ERR_DEVICE, "sample upload / check: %s", hipGetErrorString(e));
    }
    if (first < (long)n) {
        (void)hipFree(p);
        return terr(t, ETHCNN_ERR_FORMAT, "sample %zu: a QP outside 0..51, a label outside 0..3 or a non-finite vector element",
                    keep[(size_t)first]);
    }
    if (t->data[set]) (void)hipFree(t->data[set]);
    t->data[set] = (uint8_t*)p;
    t->nrec[set] = (int64_t)n;
    return 0;
}

// the same from an ETH-LSTM sample set already in HBM (include/ethcnn.h "ETH-LSTM sample sets"): the QP selection on the slot-0 QP
// floats (the only bytes that leave HBM), then the buffer adopted (take, everything kept) or a compacting device-to-device copy
extern "C" int ethcnn_lstm_train_set_samples_from(ethcnn_lstm_trainer* t, int set, ethcnn_lstm_samples* sm, int take) {
    namespace ls = ethcnn::lstm_samples;
    if (!t) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return terr(t, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    if (!sm || !sm->built || sm->count == 0) return terr(t, ETHCNN_ERR_ARG, "no sample records (the sample set is not built or empty)");
    if (sm->c != t->c) return terr(t, ETHCNN_ERR_ARG, "the sample set and the trainer live on different contexts");
    const size_t nall = (size_t)sm->count;
    hipStream_t s = t->c->stream;
    TCHK(t, hipSetDevice(t->c->device));
    TCHK(t, hipStreamSynchronize(s));
    // SELECT_QP_LIST, as in ethcnn_lstm_train_set_samples
    std::vector<int64_t> keep;
    if (t->nqps) {
        float* d_q = nullptr;
        std::vector<float> q(nall);
        hipError_t e = hipMalloc((void**)&d_q, nall * 4);
        if (e == hipSuccess) {
            ls::launch_qp0(s, sm->data, (long)nall, d_q);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(q.data(), d_q, nall * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(d_q);
        if (e != hipSuccess) return terr(t, ETHCNN_ERR_DEVICE, "sample selection: %s", hipGetErrorString(e));
        for (size_t i = 0; i < nall; ++i) {
            bool on = false;
            for (int k = 0; k < t->nqps && !on; ++k) on = q[i] == (float)t->qps[k];
            if (on) keep.push_back((int64_t)i);
        }
        if (keep.empty()) return terr(t, ETHCNN_ERR_FORMAT, "none of the %zu samples has a selected QP", nall);
    }
    const bool all = !t->nqps || keep.size() == nall;
    const size_t n = all ? nall : keep.size();
    if (n > 0x7fffffffull / kSteps) return terr(t, ETHCNN_ERR_ARG, "too many samples");
    uint8_t* p = sm->data;
    const bool adopt = all && take;
    if (!adopt) {
        if (hipMalloc((void**)&p, n * kRecBytes) != hipSuccess) {
            (void)hipGetLastError();
            return terr(t, ETHCNN_ERR_NOMEM, "%zu bytes of samples do not fit in device memory", n * kRecBytes);
        }
        hipError_t e = hipSuccess;
        int64_t* d_keep = nullptr;
        if (all) {
            e = hipMemcpyAsync(p, sm->data, n * kRecBytes, hipMemcpyDeviceToDevice, s);
        } else {
            e = hipMalloc((void**)&d_keep, n * 8);
            if (e == hipSuccess) e = hipMemcpyAsync(d_keep, keep.data(), n * 8, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) {
                ls::launch_compact(s, sm->data, d_keep, (long)n, p, t->c->cus > 0 ? t->c->cus : 256);
                e = hipGetLastError();
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (d_keep) (void)hipFree(d_keep);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return terr(t, ETHCNN_ERR_DEVICE, "sample copy: %s", hipGetErrorString(e));
        }
    }
    long first = 0;
    const hipError_t e = first_bad_sample(t, p, n, &first);
    if (e != hipSuccess || first < (long)n) {
        if (!adopt) (void)hipFree(p);
        if (e != hipSuccess) return terr(t, ETHCNN_ERR_DEVICE, "sample check: %s", hipGetErrorString(e));
        return terr(t, ETHCNN_ERR_FORMAT, "sample %lld: a QP outside 0..51, a label outside 0..3 or a non-finite vector element",
                    (long long)(all ? (int64_t)first : keep[(size_t)first]));
    }
    if (t->data[set]) (void)hipFree(t->data[set]);
    t->data[set] = p;
    t->nrec[set] = (int64_t)n;
    if (take) {  // the set is empty afterwards: its buffer is the trainer's now, or (after a compacting copy) is freed
        if (!adopt) (void)hipFree(sm->data);
        sm->data = nullptr;
        sm->count = sm->skipped = 0;
        sm->built = false;
    }
    return 0;
}

extern "C" int64_t ethcnn_lstm_train_num_samples(const ethcnn_lstm_trainer* t, int set) {
    return (t && (set == 0 || set == 1)) ? t->nrec[set] : -1;
}

extern "C" int64_t ethcnn_lstm_train_debug_rows(const ethcnn_lstm_trainer* t) { return t ? t->last_rows : -1; }

static int ready(ethcnn_lstm_trainer* t) {
    if (!t->data[ETHCNN_TRAIN_SET_TRAIN]) return terr(t, ETHCNN_ERR_ARG, "no training samples (ethcnn_lstm_train_set_samples)");
    return 0;
}

extern "C" int ethcnn_lstm_train_run(ethcnn_lstm_trainer* t, int64_t first_step, int64_t nsteps) {
    if (!t) return ETHCNN_ERR_ARG;
    if (first_step < 0 || nsteps < 0) return terr(t, ETHCNN_ERR_ARG, "negative step");
    if (int rc = ready(t)) return rc;
    TCHK(t, hipSetDevice(t->c->device));
    for (int64_t i = 0; i < nsteps; ++i)
        if (int rc = enqueue_step(t, first_step + i, false)) return rc;
    return 0;
}

extern "C" int ethcnn_lstm_train_last_stats(ethcnn_lstm_trainer* t, float loss3[3], float acc3[3]) {
    if (!t) return ETHCNN_ERR_ARG;
    TCHK(t, hipSetDevice(t->c->device));
    return read_stats(t, loss3, acc3);
}

extern "C" int ethcnn_lstm_train_step_indices(ethcnn_lstm_trainer* t, int64_t step, const int32_t* idx, int n, float loss3[3],
                                              float acc3[3]) {
    if (!t) return ETHCNN_ERR_ARG;
    if (int rc = ready(t)) return rc;
    if (!idx || n != t->B) return terr(t, ETHCNN_ERR_ARG, "an explicit batch needs %d indices", t->B);
    if (step < 0) return terr(t, ETHCNN_ERR_ARG, "negative step");
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= t->nrec[0]) return terr(t, ETHCNN_ERR_ARG, "sample index %d outside 0..%lld", idx[i], (long long)t->nrec[0] - 1);
    TCHK(t, hipSetDevice(t->c->device));
    hipStream_t s = t->c->stream;
    TCHK(t, hipMemcpyAsync(t->idx_in, idx, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    TCHK(t, hipStreamSynchronize(s));
    if (int rc = enqueue_step(t, step, true)) return rc;
    return read_stats(t, loss3, acc3);
}

extern "C" int ethcnn_lstm_train_evaluate(ethcnn_lstm_trainer* t, int set, const int32_t* idx, int64_t n, float loss3[3], float acc3[3],
                                          float* probs) {
    if (!t) return ETHCNN_ERR_ARG;
    if (set != 0 && set != 1) return terr(t, ETHCNN_ERR_ARG, "set must be 0 (train) or 1 (valid), got %d", set);
    if (!t->data[set]) return terr(t, ETHCNN_ERR_ARG, "no samples in set %d", set);
    if (n <= 0 || n > 0x7fffffffll / kOut / kSteps || (!idx && n > t->nrec[set])) return terr(t, ETHCNN_ERR_ARG, "bad sample count %lld", (long long)n);
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
    const size_t rows = (size_t)n * kSteps;
    float *Pn = nullptr, *Ln = nullptr;
    int32_t* In = nullptr;
    if (hipMalloc(&Pn, rows * kOut * 4) != hipSuccess || hipMalloc(&Ln, rows * 16 * 4) != hipSuccess ||
        hipMalloc(&In, (size_t)n * 4) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(Pn); (void)hipFree(Ln); (void)hipFree(In);
        return terr(t, ETHCNN_ERR_NOMEM, "cannot allocate the evaluation buffers of %lld samples", (long long)n);
    }
    hipError_t e = hipMemcpyAsync(In, idx, (size_t)n * 4, hipMemcpyHostToDevice, s);
    for (int64_t c0 = 0; e == hipSuccess && c0 < n; c0 += t->cap) {
        const int nb = (int)std::min<int64_t>(t->cap, n - c0);
        enqueue_forward(t, set, nb, In + c0, 0, 0, Pn + c0 * kSteps * kOut, Ln + c0 * kSteps * 16, t->g_eval, t->t_eval);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        ethcnn::train::launch_loss(s, Pn, Ln, (int)rows, t->stats, nullptr);  // ONE batch over all n x 20 rows
        e = hipGetLastError();
    }
    if (e == hipSuccess && probs) e = hipMemcpyAsync(probs, Pn, rows * kOut * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(Pn); (void)hipFree(Ln); (void)hipFree(In);
    if (e != hipSuccess) return terr(t, ETHCNN_ERR_DEVICE, "evaluation: %s", hipGetErrorString(e));
    return read_stats(t, loss3, acc3);
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
