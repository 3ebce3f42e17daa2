// ethcnn_lstm_train_kernels.hip -- the kernels of one ETH-LSTM training step and of its forward-only evaluation (exact fp32).
// Graph: ETH-LSTM_Training_LDP/net_CTU64.py:85-140 (cells and heads), :142-216 (features, labels), :256-259 (clip + momentum).
// Launch order, row layout, the time reversal and the un-reversed external features: ethcnn_lstm_train.h.  Every floating-point sum
// has a single owner (a thread or one MFMA accumulator chain) and a fixed order; no atomics.
#include <hip/hip_runtime.h>

#include "ethcnn_lstm_train.h"

namespace ethcnn {
namespace lstm_train {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));  // the kernels' blob offsets are multiples of 2 floats only
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

__device__ __constant__ const int kH[3] = {64, 128, 256}, kHOff[3] = {0, 64, 192};
__device__ __constant__ const int kN2[3] = {48, 96, 192}, kN2Off[3] = {0, 48, 144};
__device__ __constant__ const int kN3[3] = {1, 4, 16}, kN3Off[3] = {0, 1, 5};
__device__ __constant__ const int kH1Off[3] = {0, 70, 204}, kH2Off[3] = {0, 54, 156};

__device__ inline float lrelu(float x) { return x > 0.f ? x : 0.2f * x; }
__device__ inline float lrelu_grad(float a) { return a > 0.f ? 1.f : 0.2f; }
__device__ inline float sigm(float x) { return 1.f / (1.f + expf(-x)); }
__device__ inline int cell_of(int u, const int* off) { return u >= off[2] ? 2 : (u >= off[1] ? 1 : 0); }
__device__ inline float keep_mask(uint64_t seed, uint64_t step, int row, int unit, float keep) {
    const uint64_t r = draw(seed, kStreamLstmDropout, step, (uint64_t)row, (uint64_t)unit);
    return (float)(r >> 40) * (1.0f / 16777216.0f) < keep ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------ gather ---
// m: the block's entry of the member table; g: what changes from launch to launch.  keep (the member's kept records of the shared
// set, file order): sample i is record keep[i]; NULL: record i
__device__ __forceinline__ void gather_body(const LstmMember& m, const LstmGroupStep& g) {
    const LstmBufs& u = m.u;
    // (selects, not m.keep[g.set]: an index that is not a constant would put the kernel's copy of the entry into scratch memory)
    const int64_t* keep = g.set ? m.keep[1] : m.keep[0];
    const long nkept = g.set ? m.nkept[1] : m.nkept[0];
    const int row = blockIdx.x, b = row / kSteps, p = row % kSteps, t = threadIdx.x;
    long i;
    if (!g.drawn) i = m.idx_in[b];
    else i = (long)(((draw(m.seed, kStreamLstmIndex, g.step, (uint64_t)b, 0) >> 32) * (uint64_t)nkept) >> 32);
    const uint8_t* rec = g.data + (keep ? (long)keep[i] : i) * kRecBytes;
    const float* slots = (const float*)(rec + 64);  // 64 and 37264 are multiples of 4
    const float* slot = slots + p * kSlotFloats;
    for (int k = t; k < kVec; k += 128) u.X[(long)row * kVec + k] = slot[17 + k];
    if (t < 16) u.lab[(long)row * 16 + t] = slot[1 + t];
    if (t == 0) {
        if (p == 0) m.idx[b] = (int)i;
        // the features of unrolled step ts = 19 - p, which computes this row's prediction (net_CTU64.py:125): slot ts
        const int ts = kSteps - 1 - p;
        float qf = slots[ts * kSlotFloats] / 51.0f;  // :149
        if (m.qp_scale != 1.f) qf = qf * m.qp_scale;
        const long frame = (long)((uint32_t)rec[10] | (uint32_t)rec[11] << 8 | (uint32_t)rec[12] << 16 | (uint32_t)rec[13] << 24) - ts;
        const int gop = (int)(((frame % 4) + 4) % 4);  // input_data.py:113-120
        float* e = u.E + (long)row * kEf;
        e[0] = qf;
        for (int k = 0; k < 4; ++k) e[1 + k] = k == gop ? 1.f : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------ forward recurrence ---
// 256 threads = 4 waves; wave w owns the hidden-unit tiles (w + 4 i) * 16 .. + 16 and, per tile, the four gate accumulators of
// the block's 16 samples (C/D map of 16x16x4: column = lane & 15 is the unit, row = 4 (lane >> 4) + reg the sample).
template <int H>
__device__ void fwd_cell(const LstmBufs& u, const float* __restrict__ W, int kern_off, int bias_off, int xoff, float* Zc, float* HPc,
                         int nb, float* hs) {
    constexpr int NT = H / 64, G4 = 4 * H, LD = H + 4;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 15, g = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const float* U = W + kern_off + (long)H * G4;  // kernel rows H .. 2H - 1: the h_prev part of [x, h_prev] . kernel
    const float* bias = W + bias_off;
    for (int e = t; e < 16 * LD; e += 256) hs[e] = 0.f;
    for (int e = t; e < 16 * kSteps; e += 256) {
        const int b = b0 + e / kSteps;
        if (b < nb) HPc[(long)(b * kSteps + e % kSteps) * (H + 1) + H] = 1.f;
    }
    for (int e = t; e < 16 * H; e += 256) {
        const int b = b0 + e / H;
        if (b < nb) HPc[(long)(b * kSteps + kSteps - 1) * (H + 1) + e % H] = 0.f;  // zero initial state
    }
    float c[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i)
        for (int q = 0; q < 4; ++q) c[i][q] = 0.f;
    __syncthreads();
    for (int ts = 0; ts < kSteps; ++ts) {
        const int p = kSteps - 1 - ts;  // cell_inputs.reverse()
        float hn[NT][4];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int col = (w + 4 * i) * 16 + r;
            f32x4 acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int b = b0 + 4 * g + reg;
                    acc[q][reg] = b < nb ? Zc[(long)(b * kSteps + p) * G4 + q * H + col] + bias[q * H + col] : 0.f;
                }
#pragma unroll 4
            for (int k0 = 0; k0 < H; k0 += 4) {
                const float a = hs[r * LD + k0 + g];
                const float* up = U + (long)(k0 + g) * G4 + col;
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = MFMA16(a, up[q * H], acc[q]);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int b = b0 + 4 * g + reg;
                const float ig = sigm(acc[0][reg]), jg = tanhf(acc[1][reg]), fg = sigm(acc[2][reg] + 1.0f), og = sigm(acc[3][reg]);
                const float cpre = fg * c[i][reg] + ig * jg;
                const float cc = fminf(fmaxf(cpre, -5.0f), 5.0f);  // cell_clip
                const float h = og * tanhf(cc);
                c[i][reg] = cc;
                hn[i][reg] = h;
                if (b < nb) {
                    const long row = (long)b * kSteps + p;
                    float* z = Zc + row * G4 + col;
                    z[0] = ig; z[H] = jg; z[2 * H] = fg; z[3 * H] = og;
                    u.Cpre[row * kVec + xoff + col] = cpre;
                    u.C[row * kVec + xoff + col] = cc;
                    u.Hout[row * kVec + xoff + col] = h;
                    if (p > 0) HPc[(row - 1) * (H + 1) + col] = h;
                }
            }
        }
        __syncthreads();  // every wave has read this step's h_prev
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) hs[(4 * g + reg) * LD + (w + 4 * i) * 16 + r] = hn[i][reg];
        __syncthreads();
    }
}

__device__ __forceinline__ void fwd_body(const LstmBufs& u, const float* __restrict__ W, const LstmOffsets& o, const int nb) {
    __shared__ float hs[16 * 260];
    const int cell = blockIdx.y;
    if (cell == 0) fwd_cell<64>(u, W, o.kern[0], o.bias[0], 0, u.Z[0], u.HP[0], nb, hs);
    else if (cell == 1) fwd_cell<128>(u, W, o.kern[1], o.bias[1], 64, u.Z[1], u.HP[1], nb, hs);
    else fwd_cell<256>(u, W, o.kern[2], o.bias[2], 192, u.Z[2], u.HP[2], nb, hs);
}

// ------------------------------------------------------------------------------------------------------------ heads forward ---
__device__ __forceinline__ void heads_fwd_body(const LstmBufs& u, const float* __restrict__ W, const LstmOffsets& o, const uint64_t seed,
                                               const uint64_t step, const int dropout) {
    __shared__ float h1[kLdH1], h2[kLdH2];
    const int row = blockIdx.x, t = threadIdx.x;
    const float* ef = u.E + (long)row * kEf;
    for (int x = t; x < kVec; x += 256) {
        const int cl = cell_of(x, kHOff), j = x - kHOff[cl];
        const float hv = u.Hout[(long)row * kVec + x];
        const float m = dropout ? keep_mask(seed, step, row, x, 0.5f) : 1.f;
        u.M1[(long)row * kVec + x] = m;
        h1[kH1Off[cl] + j] = dropout ? (hv / 0.5f) * m : hv;  // DropoutWrapper(output_keep_prob = 0.5): x / keep * floor(keep + U)
    }
    if (t < 18) {
        const int cl = t / 6, k = t % 6;
        h1[kH1Off[cl] + kH[cl] + k] = k < 5 ? ef[k] : 1.f;
        h2[kH2Off[cl] + kN2[cl] + k] = k < 5 ? ef[k] : 1.f;
    }
    __syncthreads();
    for (int x = t; x < kLdH1; x += 256) u.H1[(long)row * kLdH1 + x] = h1[x];
    for (int v = t; v < kFc2; v += 256) {
        const int cl = cell_of(v, kN2Off), j = v - kN2Off[cl], n1 = kH[cl] + kEf, n2 = kN2[cl];
        const float* w = W + o.w2[cl];
        const float* x = h1 + kH1Off[cl];
        float acc = 0.f;
        for (int k = 0; k < n1; ++k) acc += x[k] * w[k * n2 + j];  // [h, qp, one-hot] x W2
        const float av = lrelu(acc + W[o.b2[cl] + j]);
        const float m = dropout ? keep_mask(seed, step, row, kVec + v, 0.8f) : 1.f;
        u.A2[(long)row * kFc2 + v] = av;
        u.M2[(long)row * kFc2 + v] = m;
        h2[kH2Off[cl] + j] = dropout ? (av / 0.8f) * m : av;
    }
    __syncthreads();
    for (int x = t; x < kLdH2; x += 256) u.H2[(long)row * kLdH2 + x] = h2[x];
    if (t < kOut) {
        const int cl = cell_of(t, kN3Off), j = t - kN3Off[cl], n2 = kN2[cl] + kEf, n3 = kN3[cl];
        const float* w = W + o.w3[cl];
        const float* x = h2 + kH2Off[cl];
        float acc = 0.f;
        for (int k = 0; k < n2; ++k) acc += x[k] * w[k * n3 + j];
        u.P[(long)row * kOut + t] = sigm(acc + W[o.b3[cl] + j]);
    }
}

// ----------------------------------------------------------------------------------------------------------- heads backward ---
__device__ __forceinline__ void heads_bwd_body(const LstmBufs& u, const float* __restrict__ W, const LstmOffsets& o, const int dropout) {
    __shared__ float dz3[kOut], dz2[kFc2];
    const int row = blockIdx.x, t = threadIdx.x;
    if (t < kOut) dz3[t] = u.dZ3[(long)row * kOut + t];
    __syncthreads();
    for (int v = t; v < kFc2; v += 256) {
        const int cl = cell_of(v, kN2Off), j = v - kN2Off[cl], n3 = kN3[cl];
        const float* w = W + o.w3[cl];
        float acc = 0.f;
        for (int c = 0; c < n3; ++c) acc += w[j * n3 + c] * dz3[kN3Off[cl] + c];
        const float da = dropout ? (acc * u.M2[(long)row * kFc2 + v]) / 0.8f : acc;
        const float dz = da * lrelu_grad(u.A2[(long)row * kFc2 + v]);
        dz2[v] = dz;
        u.dZ2[(long)row * kFc2 + v] = dz;
    }
    __syncthreads();
    for (int x = t; x < kVec; x += 256) {
        const int cl = cell_of(x, kHOff), j = x - kHOff[cl], n2 = kN2[cl];
        const float* w = W + o.w2[cl];
        float acc = 0.f;
        for (int c = 0; c < n2; ++c) acc += w[j * n2 + c] * dz2[kN2Off[cl] + c];
        u.dH[(long)row * kVec + x] = dropout ? (acc * u.M1[(long)row * kVec + x]) / 0.5f : acc;
    }
}

// ----------------------------------------------------------------------------------------------------- backward recurrence ---
// Slot 0 (the last unrolled step) first.  Thread t owns the elements e = t + 256 i of the block's [16 samples][H units] for the gate
// derivatives and carries their dc; wave w owns the hidden-unit tiles (w + 4 i) * 16 of dh_prev = dz x kernel[H:2H, :]^T, summed
// over the 4H gate columns in two halves (i | j, then f | o) staged through LDS.  Inside a block of 16 columns lane group g takes
// columns 4 g .. 4 g + 3 in MFMAs 0 .. 3 (one 16-byte load per operand): a fixed order.
template <int H>
__device__ void bwd_cell(const LstmBufs& u, const float* __restrict__ W, int kern_off, int xoff, const float* Gc, float* dZc, int nb,
                         float* dzs, float* dhs) {
    constexpr int NT = H / 64, G4 = 4 * H, LD = H + 4, LDZ = 2 * H + 4, NE = H / 16;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 15, g = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const float* U = W + kern_off + (long)H * G4;
    for (int e = t; e < 16 * LD; e += 256) dhs[e] = 0.f;
    float dc[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) dc[i] = 0.f;
    __syncthreads();
    for (int p = 0; p < kSteps; ++p) {
        float dz[NE][4];
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int e = t + 256 * i, sr = e / H, k = e % H, b = b0 + sr;
            dz[i][0] = dz[i][1] = dz[i][2] = dz[i][3] = 0.f;
            if (b < nb) {
                const long row = (long)b * kSteps + p;
                const float* gz = Gc + row * G4 + k;
                const float ig = gz[0], jg = gz[H], fg = gz[2 * H], og = gz[3 * H];
                const float cc = u.C[row * kVec + xoff + k], cpre = u.Cpre[row * kVec + xoff + k];
                const float cprev = p < kSteps - 1 ? u.C[(row + 1) * kVec + xoff + k] : 0.f;
                const float dh = u.dH[row * kVec + xoff + k] + dhs[sr * LD + k];
                const float th = tanhf(cc);
                const float dcc = (dh * og) * (1.f - th * th) + dc[i];
                const float dcp = (cpre >= -5.0f && cpre <= 5.0f) ? dcc : 0.f;  // clip_by_value: no gradient where c was clipped
                dz[i][0] = (dcp * jg) * (ig * (1.f - ig));
                dz[i][1] = (dcp * ig) * (1.f - jg * jg);
                dz[i][2] = (dcp * cprev) * (fg * (1.f - fg));
                dz[i][3] = (dh * th) * (og * (1.f - og));
                dc[i] = dcp * fg;
                float* d = dZc + row * G4 + k;
                d[0] = dz[i][0]; d[H] = dz[i][1]; d[2 * H] = dz[i][2]; d[3 * H] = dz[i][3];
            }
        }
        __syncthreads();  // dhs of this step is consumed
        if (p == kSteps - 1) break;  // slot 19 starts from the zero state: nothing to carry further (uniform over the block)
        f32x4 acc[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {  // unrolled: dz[][] is indexed by constants and stays in registers
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int e = t + 256 * i, sr = e / H, k = e % H;
                dzs[sr * LDZ + k] = dz[i][2 * ph];
                dzs[sr * LDZ + H + k] = dz[i][2 * ph + 1];
            }
            __syncthreads();
#pragma unroll 2
            for (int kb = 0; kb < 2 * H; kb += 16) {
                const f32x4 a4 = *(const f32x4*)&dzs[r * LDZ + kb + 4 * g];
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const int n = (w + 4 * i) * 16 + r;
                    const f32x4u b4 = *(const f32x4u*)&U[(long)n * G4 + ph * 2 * H + kb + 4 * g];
                    acc[i] = MFMA16(a4[0], b4[0], acc[i]);
                    acc[i] = MFMA16(a4[1], b4[1], acc[i]);
                    acc[i] = MFMA16(a4[2], b4[2], acc[i]);
                    acc[i] = MFMA16(a4[3], b4[3], acc[i]);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) dhs[(4 * g + reg) * LD + (w + 4 * i) * 16 + r] = acc[i][reg];
        __syncthreads();
    }
}

__device__ __forceinline__ void bwd_body(const LstmBufs& u, const float* __restrict__ W, const LstmOffsets& o, const int nb) {
    __shared__ __attribute__((aligned(16))) float dzs[16 * 516];
    __shared__ float dhs[16 * 260];
    const int cell = blockIdx.y;
    if (cell == 0) bwd_cell<64>(u, W, o.kern[0], 0, u.Z[0], u.dZ[0], nb, dzs, dhs);
    else if (cell == 1) bwd_cell<128>(u, W, o.kern[1], 64, u.Z[1], u.dZ[1], nb, dzs, dhs);
    else bwd_cell<256>(u, W, o.kern[2], 192, u.Z[2], u.dZ[2], nb, dzs, dhs);
}

// ------------------------------------------------------------------------------------------------- global norm and update ---
// level 1: block k sums the squares of floats [k chunk, (k + 1) chunk): thread t takes t, t + 256, ... in order, then a tree in LDS
__device__ __forceinline__ void norm_body(const float* __restrict__ grad, const long n, double* __restrict__ part) {
    __shared__ double red[256];
    const long chunk = (n + gridDim.x - 1) / gridDim.x, lo = (long)blockIdx.x * chunk, hi = min(n, lo + chunk);
    double s = 0.0;
    for (long j = lo + threadIdx.x; j < hi; j += 256) s += (double)grad[j] * (double)grad[j];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// level 2 (every block, the same order) + tf.clip_by_global_norm (scale = clip * min(1 / norm, 1 / clip)) + MomentumOptimizer.
// grad keeps the unclipped gradient; stats[7] = the global norm.
__device__ __forceinline__ void update_body(float* __restrict__ W, float* __restrict__ acc, const float* __restrict__ grad,
                                            const double* __restrict__ part, const int nparts, const float clip, const float lr,
                                            const float momentum, const long n, float* __restrict__ stats) {
    __shared__ float s_scale;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < nparts; ++k) s += part[k];
        const float norm = (float)sqrt(s);
        // minimum(1 / norm, 1 / clip) as a comparison that keeps its first operand: a NaN norm gives a NaN scale and so a NaN
        // update (fminf would return 1 / clip: scale 1, and the finite part of the weights would move as if nothing had happened)
        float scale = 1.f;
        if (clip > 0.f) {
            const float a = 1.f / norm, b = 1.f / clip;
            scale = clip * ((b < a) ? b : a);
        }
        s_scale = scale;
        if (blockIdx.x == 0) stats[7] = norm;
    }
    __syncthreads();
    const float scale = s_scale;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long)gridDim.x * 256) {
        const float gj = clip > 0.f ? grad[j] * scale : grad[j];
        const float a = acc[j] * momentum + gj;
        acc[j] = a;
        W[j] = W[j] - lr * a;
    }
}

// -------------------------------------------------------------------------------------------------------------- the kernels ---
// K >= 1 trainers in every launch of a step (ethcnn_lstm_train.h "the member table").  tab: the device-resident member table.  The
// member is the grid's last dimension, so blockIdx.x (and, in the recurrences, blockIdx.y = the cell) and gridDim.x do not depend on
// K or on the member; each block runs the body on its member's buffers.  The members share the sample records only.
// member_of: the block's entry, fetched once (a uniform address: scalar loads), every pointer marked as device memory
// (train::as_global), so the bodies' accesses are global_load / global_store and not FLAT ones, which would wait on the counter the
// recurrences' LDS traffic uses.
__device__ __forceinline__ LstmMember member_of(const LstmMember* __restrict__ tab, const unsigned i) {
    using train::as_global;
    const LstmMember& e = tab[i];  // in memory
    LstmMember m = e;
    LstmBufs& u = m.u;
    u.X = as_global(e.u.X); u.lab = as_global(e.u.lab); u.E = as_global(e.u.E);
    for (int c = 0; c < 3; ++c) {
        u.Z[c] = as_global(e.u.Z[c]); u.HP[c] = as_global(e.u.HP[c]); u.dZ[c] = as_global(e.u.dZ[c]);
    }
    u.Cpre = as_global(e.u.Cpre); u.C = as_global(e.u.C); u.Hout = as_global(e.u.Hout);
    u.M1 = as_global(e.u.M1); u.H1 = as_global(e.u.H1); u.A2 = as_global(e.u.A2); u.M2 = as_global(e.u.M2); u.H2 = as_global(e.u.H2);
    u.P = as_global(e.u.P); u.dZ3 = as_global(e.u.dZ3); u.dZ2 = as_global(e.u.dZ2); u.dH = as_global(e.u.dH);
    m.W = as_global(e.W); m.acc = as_global(e.acc); m.grad = as_global(e.grad); m.part = as_global(e.part);
    m.stats = as_global(e.stats); m.idx_in = as_global(e.idx_in); m.idx = as_global(e.idx);
    m.keep[0] = as_global(e.keep[0]); m.keep[1] = as_global(e.keep[1]);
    return m;
}
__global__ __launch_bounds__(128) void k_lstm_group_gather(const LstmMember* __restrict__ tab, LstmGroupStep g) {
    const LstmMember m = member_of(tab, blockIdx.y);
    gather_body(m, g);
}
__global__ __launch_bounds__(256) void k_lstm_group_fwd(const LstmMember* __restrict__ tab, LstmOffsets o, int nb) {
    const LstmMember m = member_of(tab, blockIdx.z);
    fwd_body(m.u, m.W, o, nb);
}
__global__ __launch_bounds__(256) void k_lstm_group_heads_fwd(const LstmMember* __restrict__ tab, LstmOffsets o, uint64_t step, int train) {
    const LstmMember m = member_of(tab, blockIdx.y);
    heads_fwd_body(m.u, m.W, o, m.seed, step, train ? m.dropout : 0);
}
__global__ __launch_bounds__(256) void k_lstm_group_heads_bwd(const LstmMember* __restrict__ tab, LstmOffsets o) {
    const LstmMember m = member_of(tab, blockIdx.y);
    heads_bwd_body(m.u, m.W, o, m.dropout);
}
__global__ __launch_bounds__(256) void k_lstm_group_bwd(const LstmMember* __restrict__ tab, LstmOffsets o, int nb) {
    const LstmMember m = member_of(tab, blockIdx.z);
    bwd_body(m.u, m.W, o, nb);
}
__global__ __launch_bounds__(256) void k_lstm_group_norm(const LstmMember* __restrict__ tab, long n) {
    const LstmMember m = member_of(tab, blockIdx.y);
    norm_body(m.grad, n, m.part);
}
__global__ __launch_bounds__(256) void k_lstm_group_update(const LstmMember* __restrict__ tab, train::GroupRates r, long n) {
    const LstmMember m = member_of(tab, blockIdx.y);
    update_body(m.W, m.acc, m.grad, m.part, kNormBlocks, m.clip, r.lr[blockIdx.y], m.momentum, n, m.stats);
}

// ------------------------------------------------------------------------------------------------------------- sample check ---
// a record is bad when it holds a QP that is not an integer in 0..51, a label that is not an integer in 0..3 or a vector element that
// is not finite
__device__ inline bool sample_float_ok(int c, float v) {  // float c of a slot: [qp | 16 labels | 448 vector]
    return c == 0 ? (v >= 0.f && v <= 51.f && v == truncf(v)) : (c <= 16 ? (v >= 0.f && v <= 3.f && v == truncf(v)) : isfinite(v));
}

// per listed record: bad[j] = 1 when record list[j] (NULL: j) is bad.  Every thread that finds a bad float stores the same 1: no sum,
// no order.
__global__ __launch_bounds__(256) void k_lstm_check_list(const uint8_t* __restrict__ data, const int64_t* __restrict__ list, long n,
                                                          uint8_t* __restrict__ bad) {
    __shared__ int any;
    constexpr int kF = kSlotFloats * kSteps;
    for (long j = blockIdx.x; j < n; j += gridDim.x) {
        if (threadIdx.x == 0) any = 0;
        __syncthreads();
        const float* f = (const float*)(data + (list ? (long)list[j] : j) * kRecBytes + 64);
        bool ok = true;
        for (int e = threadIdx.x; e < kF; e += 256) ok = ok && sample_float_ok(e % kSlotFloats, f[e]);
        if (!ok) any = 1;
        __syncthreads();
        if (threadIdx.x == 0) bad[j] = (uint8_t)any;
        __syncthreads();
    }
}

// --------------------------------------------------------------------------------------------------------------- launchers ---
void launch_check_list(hipStream_t s, const uint8_t* data, const int64_t* list, long n, uint8_t* bad, int nblocks) {
    hipLaunchKernelGGL(k_lstm_check_list, dim3(nblocks), dim3(256), 0, s, data, list, n, bad);
}

// the launches of a step, each over all k members
void launch_group_gather(hipStream_t s, int nb, int k, const LstmMember* tab, const LstmGroupStep& g) {
    hipLaunchKernelGGL(k_lstm_group_gather, dim3(nb * kSteps, k), dim3(128), 0, s, tab, g);
}
void launch_group_fwd(hipStream_t s, int nb, int k, const LstmMember* tab, const LstmOffsets& o) {
    hipLaunchKernelGGL(k_lstm_group_fwd, dim3((nb + 15) / 16, 3, k), dim3(256), 0, s, tab, o, nb);
}
void launch_group_heads_fwd(hipStream_t s, int nb, int k, const LstmMember* tab, const LstmOffsets& o, uint64_t step, int train) {
    hipLaunchKernelGGL(k_lstm_group_heads_fwd, dim3(nb * kSteps, k), dim3(256), 0, s, tab, o, step, train);
}
void launch_group_heads_bwd(hipStream_t s, int nb, int k, const LstmMember* tab, const LstmOffsets& o) {
    hipLaunchKernelGGL(k_lstm_group_heads_bwd, dim3(nb * kSteps, k), dim3(256), 0, s, tab, o);
}
void launch_group_bwd(hipStream_t s, int nb, int k, const LstmMember* tab, const LstmOffsets& o) {
    hipLaunchKernelGGL(k_lstm_group_bwd, dim3((nb + 15) / 16, 3, k), dim3(256), 0, s, tab, o, nb);
}
void launch_group_norm_update(hipStream_t s, int k, const LstmMember* tab, const train::GroupRates& r, long n) {
    hipLaunchKernelGGL(k_lstm_group_norm, dim3(kNormBlocks, k), dim3(256), 0, s, tab, n);
    hipLaunchKernelGGL(k_lstm_group_update, dim3(1024, k), dim3(256), 0, s, tab, r, n);
}

}  // namespace lstm_train
}  // namespace ethcnn
