// ethcnn_train_kernels.hip -- the kernels of one ETH-CNN training step and of the forward-only evaluation pass (exact fp32).
// Graph, labels, loss and optimiser: ETH-CNN_Training_AI/net_CTU64.py:94-206.  Launch order and the determinism
// rule: ethcnn_train.h.  Every floating-point sum has a single owner thread (or one MFMA accumulator chain) and a fixed order.
#include <hip/hip_runtime.h>

#include "ethcnn_train.h"

namespace ethcnn {
namespace train {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __constant__ const int kHN1[3] = {64, 128, 256}, kHN2[3] = {48, 96, 192}, kHN3[3] = {1, 4, 16};
__device__ __constant__ const int kHOff1[3] = {0, 64, 192}, kHOff2[3] = {0, 48, 144}, kHOff3[3] = {0, 1, 5};
constexpr int kLdH1 = 454, kLdH2 = 342;  // per head [activations | qp | 1]
__device__ __constant__ const int kH1Off[3] = {0, 66, 196}, kH2Off[3] = {0, 50, 148};
// branch geometry, order S, M, L: side, offset of the image / conv1 output in the trunk record, F offsets of conv3 / conv2 outputs
__device__ __constant__ const int kSide[3] = {64, 32, 16}, kImgOff[3] = {0, 4096, 5120};
__device__ __constant__ const int kF3Off[3] = {0, 512, 640}, kF2Off[3] = {672, 2208, 2592};

__device__ inline float lrelu(float x) { return x > 0.f ? x : 0.2f * x; }
__device__ inline float lrelu_grad(float a) { return a > 0.f ? 1.f : 0.2f; }  // sign(leaky(x)) == sign(x): the output decides
__device__ inline int head_of(int u, const int* off) { return u >= off[2] ? 2 : (u >= off[1] ? 1 : 0); }
__device__ inline float keep_mask(uint64_t seed, uint64_t step, int slot, int unit, float keep) {
    const uint64_t r = draw(seed, kStreamDropout, step, (uint64_t)slot, (uint64_t)unit);
    return (float)(r >> 40) * (1.0f / 16777216.0f) < keep ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------------------------------ trunk forward ---
// NET = kNetAi: a 4992-byte record, luma * (1/255), the label row of QP q at 4160 + 16 q.  NET = kNetLdp: a 16516-byte record, the
// slot of QP q (g.slot_of_qp) holds [qp | 16 labels | 4096 residual bytes] at 64 + 4113 slot, residual (x - 128) / 255 * 10.
// The step kernels' bodies are device functions; the kernels ("the kernels" below) only decide whose buffers a block works on.
// m: the block's entry of the member table; g: what changes from launch to launch.
template <int NET>
__device__ __forceinline__ void trunk_fwd_body(const int b, const Member& m, const GroupStep& g, const NetOffsets& o) {
    __shared__ float rec[kTrunkRec];  // images then conv1 outputs (trunk record layout)
    __shared__ float feat[kTF];
    __shared__ float mean[21];
    __shared__ int sidx, sqp;
    // the table's pointers are device memory (as_global, ethcnn_train.h)
    const float* __restrict__ W = as_global(m.W);
    float* const lab = as_global(m.lab);
    const int t = threadIdx.x;
    if (t == 0) {
        int64_t i;
        if (!g.drawn) i = as_global(m.idx_in)[b];
        else i = (int64_t)(((draw(m.seed, kStreamIndex, g.step, (uint64_t)b, 0) >> 32) * (uint64_t)g.nrec) >> 32);
        int q;
        if (m.qp_fixed >= 0) q = m.qp_fixed;
        else if (!g.drawn && m.qp_in) q = as_global(m.qp_in)[b];
        else q = m.qps[((draw(m.seed, kStreamQp, g.step, (uint64_t)b, 0) >> 32) * (uint64_t)m.nqps) >> 32];
        sidx = (int)i;
        sqp = q;
        as_global(m.idx)[b] = (int)i;
        as_global(m.qp)[b] = q;
    }
    __syncthreads();
    if (NET == kNetAi) {
        const uint8_t* r = g.data + (int64_t)sidx * kRec;
        if (t < 16) lab[b * 16 + t] = (float)r[kLabelBase + 16 * sqp + t];
        const float inv255 = (float)(1.0 / 255.0);  // tf.scalar_mul(1.0 / 255.0, x)
        for (int p = t; p < 4096; p += 256) rec[p] = (float)r[p] * inv255;
    } else {
        // the slot base is odd (64 + 4113 slot), so the residual at +17 has no alignment: byte loads only
        const uint8_t* r = g.data + (int64_t)sidx * kRecLdp + kSlotBase + (int64_t)kSlotBytes * g.slot_of_qp[sqp];
        if (t < 16) lab[b * 16 + t] = (float)r[1 + t];
        for (int p = t; p < 4096; p += 256) rec[p] = (((float)r[17 + p] - 128.f) / 255.f) * 10.f;  // net_CTU64.py:102, in TF's order
    }
    __syncthreads();
    // aver_pool(x, 2) / aver_pool(x, 4) (net_CTU64.py:131,125)
    for (int p = t; p < 1024 + 256; p += 256) {
        const int br = p < 1024 ? 1 : 2, q = br == 1 ? p : p - 1024, k = br == 1 ? 2 : 4, s = kSide[br];
        const int y = q / s, x = q % s;
        float acc = 0.f;
        for (int dy = 0; dy < k; ++dy)
            for (int dx = 0; dx < k; ++dx) acc += rec[(y * k + dy) * 64 + x * k + dx];
        rec[kImgOff[br] + q] = acc / (float)(k * k);
    }
    __syncthreads();
    // zero_mean_norm_local(., side, 16): the mean of each 16x16 block (S 16 blocks, M 4, L 1)
    if (t < 21) {
        const int br = t < 16 ? 0 : (t < 20 ? 1 : 2), blk = t < 16 ? t : (t < 20 ? t - 16 : 0), s = kSide[br], nb = s / 16;
        const float* im = rec + kImgOff[br];
        const int by = blk / nb, bx = blk % nb;
        float acc = 0.f;
        for (int y = 0; y < 16; ++y)
            for (int x = 0; x < 16; ++x) acc += im[(by * 16 + y) * s + bx * 16 + x];
        mean[t] = acc * (1.0f / 256.0f);
    }
    __syncthreads();
    for (int p = t; p < 5376; p += 256) {
        const int br = p < 4096 ? 0 : (p < 5120 ? 1 : 2), q = p - kImgOff[br], s = kSide[br], nb = s / 16;
        const int blk = ((q / s) / 16) * nb + (q % s) / 16;
        rec[p] = rec[p] - mean[(br == 0 ? 0 : (br == 1 ? 16 : 20)) + blk];
    }
    __syncthreads();
    // conv1: 4x4 stride 4, 1 -> 16 (non_overlap_conv, net_CTU64.py:84-90), leaky-ReLU
    for (int p = t; p < 5376; p += 256) {
        const int br = p < 4096 ? 0 : (p < 5120 ? 1 : 2), q = p - kImgOff[br], s = kSide[br], so = s / 4;
        const int co = q & 15, px = q >> 4, oy = px / so, ox = px % so;
        const float* im = rec + kImgOff[br];
        const float* w = W + o.convw[br][0];
        float acc = 0.f;
        for (int ky = 0; ky < 4; ++ky)
            for (int kx = 0; kx < 4; ++kx) acc += im[(oy * 4 + ky) * s + ox * 4 + kx] * w[(ky * 4 + kx) * 16 + co];
        rec[5376 + p] = lrelu(acc + W[o.convb[br][0] + co]);
    }
    __syncthreads();
    // conv2: 2x2 stride 2, 16 -> 24, into the F layout (h_conv_flat, net_CTU64.py:162)
    for (int p = t; p < 2016; p += 256) {
        const int br = p < 1536 ? 0 : (p < 1920 ? 1 : 2), q = p - (br == 0 ? 0 : (br == 1 ? 1536 : 1920));
        const int si = kSide[br] / 4, so = si / 2, co = q % 24, px = q / 24, oy = px / so, ox = px % so;
        const float* in = rec + 5376 + kImgOff[br];
        const float* w = W + o.convw[br][1];
        float acc = 0.f;
        for (int ky = 0; ky < 2; ++ky)
            for (int kx = 0; kx < 2; ++kx)
                for (int ci = 0; ci < 16; ++ci) acc += in[((oy * 2 + ky) * si + ox * 2 + kx) * 16 + ci] * w[((ky * 2 + kx) * 16 + ci) * 24 + co];
        feat[kF2Off[br] + q] = lrelu(acc + W[o.convb[br][1] + co]);
    }
    __syncthreads();
    // conv3: 2x2 stride 2, 24 -> 32
    for (int p = t; p < 672; p += 256) {
        const int br = p < 512 ? 0 : (p < 640 ? 1 : 2), q = p - kF3Off[br];
        const int si = kSide[br] / 8, so = si / 2, co = q & 31, px = q >> 5, oy = px / so, ox = px % so;
        const float* in = feat + kF2Off[br];
        const float* w = W + o.convw[br][2];
        float acc = 0.f;
        for (int ky = 0; ky < 2; ++ky)
            for (int kx = 0; kx < 2; ++kx)
                for (int ci = 0; ci < 24; ++ci) acc += in[((oy * 2 + ky) * si + ox * 2 + kx) * 24 + ci] * w[((ky * 2 + kx) * 24 + ci) * 32 + co];
        feat[kF3Off[br] + q] = lrelu(acc + W[o.convb[br][2] + co]);
    }
    __syncthreads();
    float* tr = as_global(m.trunk) + (int64_t)b * kTrunkRec;
    for (int p = t; p < kTrunkRec; p += 256) tr[p] = rec[p];
    float* f = as_global(m.F) + (int64_t)b * kLdF;
    for (int p = t; p < kTF; p += 256) f[p] = feat[p];
    if (t == 0) f[kTF] = 1.f;  // ones column: the bias row of dW1 = F_aug^T dZ1
}

// ------------------------------------------------------------------------------------------------------------ grouped GEMM ---
// 64 x 64 output tile per block, 4 waves of 32 x 32 (v_mfma_f32_32x32x2_f32), K in steps of 32 staged through LDS
__device__ __forceinline__ void gemm_body(const GemmGroup* __restrict__ grp, const int bid) {
    __shared__ float As[32][65], Bs[32][65];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
    int gi = 0;
    const int n = grp->n;
    while (gi + 1 < n && bid >= grp->d[gi + 1].tile_begin) ++gi;
    const GemmDesc& d = grp->d[gi];
    const int tile = bid - d.tile_begin, m0 = (tile / d.tiles_n) * 64, n0 = (tile % d.tiles_n) * 64;
    const int M = d.M, N = d.N, K = d.K;
    const bool a_kfast = d.sak == 1;
    f32x16 acc;
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 32) {
        int s = 0;
        while (s + 1 < d.nseg && k0 >= d.kseg[s + 1]) ++s;
        const float* Bp = d.B[s];
        const long sbk = d.sbk[s], sbn = d.sbn[s];
        const int kb = d.kseg[s];
        const bool b_nfast = sbn == 1;
        for (int i = 0; i < 8; ++i) {
            const int e = t + 256 * i;
            const int kk = a_kfast ? (e & 31) : (e >> 6), mm = a_kfast ? (e >> 5) : (e & 63);
            const int m = m0 + mm, k = k0 + kk;
            As[kk][mm] = (m < M && k < K) ? d.A[(long)m * d.sam + (long)k * d.sak] : 0.f;
            const int kk2 = b_nfast ? (e >> 6) : (e & 31), nn = b_nfast ? (e & 63) : (e >> 5);
            const int nc = n0 + nn, k2 = k0 + kk2;
            Bs[kk2][nn] = (nc < N && k2 < K) ? Bp[(long)(k2 - kb) * sbk + (long)nc * sbn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const float av = As[2 * ks + (lane >> 5)][wm * 32 + (lane & 31)];
            const float bv = Bs[2 * ks + (lane >> 5)][wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col = lane & 31;
        const int gm = m0 + wm * 32 + row, gn = n0 + wn * 32 + col;
        if (gm < M && gn < N) {
            float* dst = gm < d.msplit ? d.C + (long)gm * d.ldc + gn : d.C2 + (long)(gm - d.msplit) * d.ldc + gn;
            *dst = acc[r];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ heads forward ---
struct HeadBufs {
    const float* Z1;  // [B][448] FC1 without bias
    float *A1, *M1, *H1, *A2, *M2, *H2, *P;
    const int32_t* qp;
};

template <int NET>
__device__ __forceinline__ void heads_fwd_body(const int b, const HeadBufs& h, const float* __restrict__ W, const NetOffsets& o,
                                               const uint64_t seed, const uint64_t step, const int dropout) {
    __shared__ float h1[kLdH1], h2[kLdH2];
    const int t = threadIdx.x;
    const float qpf = NET == kNetAi ? (float)h.qp[b] * (float)(1.0 / 51.0)   // tf.scalar_mul(1 / 51.0, qp)
                                    : ((float)h.qp[b] / 51.f) * 0.18f;       // LDP net_CTU64.py:103
    for (int u = t; u < kTV; u += 256) {
        const int hd = head_of(u, kHOff1), j = u - kHOff1[hd];
        const float av = lrelu(h.Z1[(long)b * kTV + u] + W[o.b1[hd] + j]);
        const float m = dropout ? keep_mask(seed, step, b, u, 0.5f) : 1.f;
        const float v = dropout ? (av / 0.5f) * m : av;  // tf.nn.dropout: x / keep_prob * floor(keep_prob + U)
        h.A1[(long)b * kTV + u] = av;
        h.M1[(long)b * kTV + u] = m;
        h1[kH1Off[hd] + j] = v;
    }
    if (t < 3) {
        h1[kH1Off[t] + kHN1[t]] = qpf;
        h1[kH1Off[t] + kHN1[t] + 1] = 1.f;
    }
    __syncthreads();
    for (int u = t; u < kLdH1; u += 256) h.H1[(long)b * kLdH1 + u] = h1[u];
    for (int v = t; v < kT2; v += 256) {
        const int hd = head_of(v, kHOff2), j = v - kHOff2[hd], n1 = kHN1[hd], n2 = kHN2[hd];
        const float* w = W + o.w2[hd];
        const float* x = h1 + kH1Off[hd];
        float acc = 0.f;
        for (int k = 0; k <= n1; ++k) acc += x[k] * w[k * n2 + j];  // [h_fc1, qp] x W2
        const float av = lrelu(acc + W[o.b2[hd] + j]);
        const float m = dropout ? keep_mask(seed, step, b, kTV + v, 0.8f) : 1.f;
        const float val = dropout ? (av / 0.8f) * m : av;
        h.A2[(long)b * kT2 + v] = av;
        h.M2[(long)b * kT2 + v] = m;
        h2[kH2Off[hd] + j] = val;
    }
    if (t < 3) {
        h2[kH2Off[t] + kHN2[t]] = qpf;
        h2[kH2Off[t] + kHN2[t] + 1] = 1.f;
    }
    __syncthreads();
    for (int u = t; u < kLdH2; u += 256) h.H2[(long)b * kLdH2 + u] = h2[u];
    if (t < kTOut) {
        const int hd = head_of(t, kHOff3), j = t - kHOff3[hd], n2 = kHN2[hd], n3 = kHN3[hd];
        const float* w = W + o.w3[hd];
        const float* x = h2 + kH2Off[hd];
        float acc = 0.f;
        for (int k = 0; k <= n2; ++k) acc += x[k] * w[k * n3 + j];
        const float z = acc + W[o.b3[hd] + j];
        h.P[(long)b * kTOut + t] = 1.f / (1.f + expf(-z));
    }
}

// ------------------------------------------------------------------------------------------------------------ loss ---
// labels of element e of a sample (net_CTU64.py:97-111): level 0 = 64x64 (1), 1 = 32x32 (4), 2 = 16x16 (16)
__device__ inline void label_of(const float* d, int e, float& y, float& valid, int& level) {
    const auto relu = [](float v) { return v > 0.f ? v : 0.f; };
    if (e == 0) {
        float s = 0.f;
        for (int i = 0; i < 16; ++i) s += d[i];
        const float av = s / 16.f;
        y = relu(av - 0.f) - relu(av - 1.f);
        valid = 1.f;
        level = 0;
    } else if (e < 5) {
        const int q = e - 1, by = q >> 1, bx = q & 1;
        const float s = d[(2 * by) * 4 + 2 * bx] + d[(2 * by) * 4 + 2 * bx + 1] + d[(2 * by + 1) * 4 + 2 * bx] + d[(2 * by + 1) * 4 + 2 * bx + 1];
        const float av = s / 4.f;
        y = relu(av - 1.f) - relu(av - 2.f);
        valid = relu(av - 0.f) - relu(av - 1.f);
        level = 1;
    } else {
        const float v = d[e - 5];
        y = relu(v - 2.f);
        valid = relu(v - 1.f) - relu(v - 2.f);
        level = 2;
    }
}

// stats: [0..2] loss_list (64, 32, 16), [3..5] accuracy_list, [6] total_loss.  dZ (may be NULL): dL/dlogit [n][21].
__device__ __forceinline__ void loss_body(const float* __restrict__ P, const float* __restrict__ lab, const int n, float* stats,
                                          float* dZ) {
    constexpr int kQ = 18;  // per level: pos sum, neg sum, #pos, #neg, accuracy numerator, accuracy denominator
    __shared__ double red[kQ][256];
    __shared__ float fin[kQ];
    const int t = threadIdx.x;
    double q[kQ];
    for (int i = 0; i < kQ; ++i) q[i] = 0.0;
    const long total = (long)n * kTOut;
    for (int sm = t; sm < n; sm += 256) {  // a sample per iteration; unrolled, so every q[] index is a constant (no scratch)
#pragma unroll
        for (int e = 0; e < kTOut; ++e) {
            float y, valid;
            int lv;
            label_of(lab + (long)sm * 16, e, y, valid, lv);
            const float p = P[(long)sm * kTOut + e];
            const float pos = -(y * logf(p + 1e-12f)) * valid, neg = -((1.f - y) * logf((1.f - p) + 1e-12f)) * valid;
            q[lv * 6 + 0] += pos;
            q[lv * 6 + 1] += neg;
            q[lv * 6 + 2] += (lv == 0 ? y : y * valid) != 0.f ? 1.0 : 0.0;
            q[lv * 6 + 3] += (lv == 0 ? 1.f - y : (1.f - y) * valid) != 0.f ? 1.0 : 0.0;
            const float eq = rintf(p) == rintf(y) ? 1.f : 0.f;  // tf.round: half to even
            q[lv * 6 + 4] += lv == 0 ? eq : valid * (valid * eq);
            q[lv * 6 + 5] += lv == 0 ? 1.0 : valid;
        }
    }
    for (int i = 0; i < kQ; ++i) red[i][t] = q[i];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w)
            for (int i = 0; i < kQ; ++i) red[i][t] += red[i][t + w];
        __syncthreads();
    }
    if (t < kQ) fin[t] = (float)red[t][0];
    __syncthreads();
    if (t == 0) {
        float tl = 0.f;
        for (int lv = 0; lv < 3; ++lv) {
            const float* f = fin + lv * 6;
            const float l = (f[0] / (f[2] + 1e-12f) + f[1] / (f[3] + 1e-12f)) / 2.f;
            stats[lv] = l;
            stats[3 + lv] = lv == 0 ? f[4] / f[5] : f[4] / (f[5] + 1e-12f);
            tl += l;
        }
        stats[6] = stats[2] + stats[1] + stats[0];  // loss_16 + loss_32 + loss_64
        (void)tl;
    }
    if (!dZ) return;
    for (long i = t; i < total; i += 256) {
        const int s = (int)(i / kTOut), e = (int)(i % kTOut);
        float y, valid;
        int lv;
        label_of(lab + (long)s * 16, e, y, valid, lv);
        const float p = P[i];
        const float cp = fin[lv * 6 + 2] + 1e-12f, cn = fin[lv * 6 + 3] + 1e-12f;
        // d/dp of (sum(-y log(p + eps) v) / cp + sum(-(1 - y) log((1 - p) + eps) v) / cn) / 2
        const float gpos = -(y * valid) / (p + 1e-12f) / cp, gneg = ((1.f - y) * valid) / ((1.f - p) + 1e-12f) / cn;
        const float gp = (gpos + gneg) * 0.5f;
        dZ[i] = gp * p * (1.f - p);  // SigmoidGrad: dy * y * (1 - y)
    }
}

// ------------------------------------------------------------------------------------------------------------ heads backward ---
struct HeadGrads {
    const float *dZ3, *A1, *M1, *A2, *M2;
    float *dZ2, *dZ1;
};

__device__ __forceinline__ void heads_bwd_body(const int b, const HeadGrads& g, const float* __restrict__ W, const NetOffsets& o,
                                               const int dropout) {
    __shared__ float dz3[kTOut], dz2[kT2];
    const int t = threadIdx.x;
    if (t < kTOut) dz3[t] = g.dZ3[(long)b * kTOut + t];
    __syncthreads();
    for (int v = t; v < kT2; v += 256) {
        const int hd = head_of(v, kHOff2), j = v - kHOff2[hd], n3 = kHN3[hd];
        const float* w = W + o.w3[hd];
        float acc = 0.f;
        for (int c = 0; c < n3; ++c) acc += w[j * n3 + c] * dz3[kHOff3[hd] + c];
        const float da = dropout ? (acc * g.M2[(long)b * kT2 + v]) / 0.8f : acc;
        const float dz = da * lrelu_grad(g.A2[(long)b * kT2 + v]);
        dz2[v] = dz;
        g.dZ2[(long)b * kT2 + v] = dz;
    }
    __syncthreads();
    for (int u = t; u < kTV; u += 256) {
        const int hd = head_of(u, kHOff1), j = u - kHOff1[hd], n2 = kHN2[hd];
        const float* w = W + o.w2[hd];
        float acc = 0.f;
        for (int c = 0; c < n2; ++c) acc += w[j * n2 + c] * dz2[kHOff2[hd] + c];
        const float da = dropout ? (acc * g.M1[(long)b * kTV + u]) / 0.5f : acc;
        g.dZ1[(long)b * kTV + u] = da * lrelu_grad(g.A1[(long)b * kTV + u]);
    }
}

// ------------------------------------------------------------------------------------------------------------ trunk backward ---
// per-sample partial gradients of the 18 conv tensors, written at their blob offsets: part[b][0 .. kConvFloats)
__device__ __forceinline__ void trunk_bwd_body(const int b, const float* __restrict__ trunk, const float* __restrict__ F,
                                               const float* __restrict__ dF, const float* __restrict__ W, const NetOffsets& o,
                                               float* __restrict__ part) {
    __shared__ float d3[672], d2[2016], d1[5376];
    const int t = threadIdx.x;
    const float* tr = trunk + (long)b * kTrunkRec;
    const float* f = F + (long)b * kLdF;
    const float* df = dF + (long)b * kTF;
    float* pg = part + (long)b * kConvFloats;
    for (int p = t; p < 672; p += 256) d3[p] = df[p] * lrelu_grad(f[p]);
    __syncthreads();
    // conv3 weights / bias, and d(conv2 output) = W3-scatter of d3 + the direct feature gradient
    for (int p = t; p < 3 * (3072 + 32); p += 256) {
        const int br = p / 3104, q = p % 3104, s3 = kSide[br] / 16, s2 = kSide[br] / 8;
        const float* dd = d3 + kF3Off[br];
        float acc = 0.f;
        if (q < 3072) {
            const int co = q & 31, ci = (q >> 5) % 24, kk = q / 768, ky = kk >> 1, kx = kk & 1;
            const float* in = f + kF2Off[br];
            for (int y = 0; y < s3; ++y)
                for (int x = 0; x < s3; ++x) acc += in[((y * 2 + ky) * s2 + x * 2 + kx) * 24 + ci] * dd[(y * s3 + x) * 32 + co];
            pg[o.convw[br][2] + q] = acc;
        } else {
            const int co = q - 3072;
            for (int px = 0; px < s3 * s3; ++px) acc += dd[px * 32 + co];
            pg[o.convb[br][2] + co] = acc;
        }
    }
    for (int p = t; p < 2016; p += 256) {
        const int br = p < 1536 ? 0 : (p < 1920 ? 1 : 2), q = p - (kF2Off[br] - 672), s2 = kSide[br] / 8, s3 = s2 / 2;
        const int ci = q % 24, px = q / 24, iy = px / s2, ix = px % s2, ky = iy & 1, kx = ix & 1;
        const float* w = W + o.convw[br][2] + ((ky * 2 + kx) * 24 + ci) * 32;
        const float* dd = d3 + kF3Off[br] + ((iy >> 1) * s3 + (ix >> 1)) * 32;
        float acc = 0.f;
        for (int co = 0; co < 32; ++co) acc += w[co] * dd[co];
        acc = acc + df[kF2Off[br] + q];
        d2[p] = acc * lrelu_grad(f[kF2Off[br] + q]);
    }
    __syncthreads();
    // conv2 weights / bias, and d(conv1 output)
    for (int p = t; p < 3 * (1536 + 24); p += 256) {
        const int br = p / 1560, q = p % 1560, s2 = kSide[br] / 8, s1 = kSide[br] / 4;
        const float* dd = d2 + (kF2Off[br] - 672);
        float acc = 0.f;
        if (q < 1536) {
            const int co = q % 24, ci = (q / 24) & 15, kk = q / 384, ky = kk >> 1, kx = kk & 1;
            const float* in = tr + 5376 + kImgOff[br];
            for (int y = 0; y < s2; ++y)
                for (int x = 0; x < s2; ++x) acc += in[((y * 2 + ky) * s1 + x * 2 + kx) * 16 + ci] * dd[(y * s2 + x) * 24 + co];
            pg[o.convw[br][1] + q] = acc;
        } else {
            const int co = q - 1536;
            for (int px = 0; px < s2 * s2; ++px) acc += dd[px * 24 + co];
            pg[o.convb[br][1] + co] = acc;
        }
    }
    for (int p = t; p < 5376; p += 256) {
        const int br = p < 4096 ? 0 : (p < 5120 ? 1 : 2), q = p - kImgOff[br], s1 = kSide[br] / 4, s2 = s1 / 2;
        const int ci = q & 15, px = q >> 4, iy = px / s1, ix = px % s1, ky = iy & 1, kx = ix & 1;
        const float* w = W + o.convw[br][1] + ((ky * 2 + kx) * 16 + ci) * 24;
        const float* dd = d2 + (kF2Off[br] - 672) + ((iy >> 1) * s2 + (ix >> 1)) * 24;
        float acc = 0.f;
        for (int co = 0; co < 24; ++co) acc += w[co] * dd[co];
        d1[p] = acc * lrelu_grad(tr[5376 + p]);
    }
    __syncthreads();
    // conv1 weights / bias (the input: the mean-removed branch image)
    for (int p = t; p < 3 * (256 + 16); p += 256) {
        const int br = p / 272, q = p % 272, s = kSide[br], s1 = s / 4;
        const float* dd = d1 + kImgOff[br];
        float acc = 0.f;
        if (q < 256) {
            const int co = q & 15, kk = q >> 4, ky = kk >> 2, kx = kk & 3;
            const float* im = tr + kImgOff[br];
            for (int y = 0; y < s1; ++y)
                for (int x = 0; x < s1; ++x) acc += im[(y * 4 + ky) * s + x * 4 + kx] * dd[(y * s1 + x) * 16 + co];
            pg[o.convw[br][0] + q] = acc;
        } else {
            const int co = q - 256;
            for (int px = 0; px < s1 * s1; ++px) acc += dd[px * 16 + co];
            pg[o.convb[br][0] + co] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ update ---
// MomentumOptimizer (use_nesterov=False): accum = accum * momentum + grad; var -= lr * accum.  Conv gradients: sum of the
// per-sample partials in sample order.  mask.n > 0 (PARTLY_TUNING_MODE 1..3): only the blob ranges [lo, hi) are optimised; every
// other weight and its accumulator is left untouched (not even rewritten).
__device__ __forceinline__ void update_body(float* __restrict__ W, float* __restrict__ acc, float* __restrict__ grad,
                                            const float* __restrict__ part, const int nb, const float lr, const float momentum,
                                            const long n, const TuneMask& mask) {
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long)gridDim.x * 256) {
        if (mask.n) {
            bool on = false;
            for (int r = 0; r < mask.n; ++r) on = on || (j >= mask.lo[r] && j < mask.hi[r]);
            if (!on) continue;
        }
        float g;
        if (j < kConvFloats) {
            g = 0.f;
            for (int b = 0; b < nb; ++b) g += part[(long)b * kConvFloats + j];
            grad[j] = g;
        } else {
            g = grad[j];
        }
        const float a = acc[j] * momentum + g;
        acc[j] = a;
        W[j] = W[j] - lr * a;
    }
}

// ------------------------------------------------------------------------------------------------------------ the kernels ---
// K >= 1 trainers in every launch of a step (ethcnn_train.h "the member table").  tab: the device-resident member table; grid (B, K)
// for the per-sample kernels, K blocks for the loss, K x tiles for the GEMMs, (1024, K) for the update.  Each block runs the body on
// its member's buffers; the members share only the sample records.  G: a pointer read from the table is device memory (as_global,
// ethcnn_train.h), so the bodies get global_load / global_store as they would for a by-value argument, not FLAT accesses.
#define G(p) as_global(p)
template <int NET>
__global__ __launch_bounds__(256) void k_group_trunk_fwd(const Member* __restrict__ tab, GroupStep g, NetOffsets o) {
    trunk_fwd_body<NET>(blockIdx.x, tab[blockIdx.y], g, o);
}
// the members' descriptor groups side by side: every member has the same shapes, hence the same tile count
__global__ __launch_bounds__(256) void k_group_gemm(const GemmGroup* __restrict__ grps, int tiles_per) {
    gemm_body(grps + blockIdx.x / tiles_per, blockIdx.x % tiles_per);
}
template <int NET>
__global__ __launch_bounds__(256) void k_group_heads_fwd(const Member* __restrict__ tab, NetOffsets o, uint64_t step) {
    const Member& m = tab[blockIdx.y];
    const HeadBufs h{G(m.Z1), G(m.A1), G(m.M1), G(m.H1), G(m.A2), G(m.M2), G(m.H2), G(m.P), G(m.qp)};
    heads_fwd_body<NET>(blockIdx.x, h, G(m.W), o, m.seed, step, m.dropout);
}
__global__ __launch_bounds__(256) void k_group_loss(const Member* __restrict__ tab, int n, int with_grad) {
    const Member& m = tab[blockIdx.x];
    loss_body(G(m.P), G(m.lab), n, G(m.stats), with_grad ? G(m.dZ3) : nullptr);
}
__global__ __launch_bounds__(256) void k_group_heads_bwd(const Member* __restrict__ tab, NetOffsets o) {
    const Member& m = tab[blockIdx.y];
    const HeadGrads g{G(m.dZ3), G(m.A1), G(m.M1), G(m.A2), G(m.M2), G(m.dZ2), G(m.dZ1)};
    heads_bwd_body(blockIdx.x, g, G(m.W), o, m.dropout);
}
__global__ __launch_bounds__(256) void k_group_trunk_bwd(const Member* __restrict__ tab, NetOffsets o) {
    const Member& m = tab[blockIdx.y];
    trunk_bwd_body(blockIdx.x, G(m.trunk), G(m.F), G(m.dF), G(m.W), o, G(m.part));
}
__global__ __launch_bounds__(256) void k_group_update(const Member* __restrict__ tab, int nb, GroupRates r, long n, TuneMask mask) {
    const Member& m = tab[blockIdx.y];
    update_body(G(m.W), G(m.acc), G(m.grad), G(m.part), nb, r.lr[blockIdx.y], m.momentum, n, mask);
}
#undef G

// ------------------------------------------------------------------------------------------------------------ LDP set check ---
// first record (per block, over a contiguous range of records) whose four slot QP bytes differ from `want` (record 0's, packed
// little-endian); nrec when there is none.  A min over the block in LDS, no atomics: the host takes the min over the blocks.
__global__ __launch_bounds__(256) void k_train_check_slots(const uint8_t* __restrict__ data, long nrec, uint32_t want,
                                                            long* __restrict__ first_bad) {
    __shared__ long red[256];
    const long per = (nrec + gridDim.x - 1) / gridDim.x, r0 = (long)blockIdx.x * per, r1 = min(nrec, r0 + per);
    long bad = nrec;
    for (long i = r0 + threadIdx.x; i < r1 && bad == nrec; i += 256) {
        const uint8_t* r = data + i * kRecLdp + kSlotBase;
        uint32_t got = 0;
        for (int q = 0; q < 4; ++q) got |= (uint32_t)r[(long)kSlotBytes * q] << (8 * q);
        if (got != want) bad = i;
    }
    red[threadIdx.x] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) first_bad[blockIdx.x] = red[0];
}

// ------------------------------------------------------------------------------------------------------------ launchers ---
void launch_check_slots(hipStream_t s, const uint8_t* data, long nrec, uint32_t want, long* first_bad, int nblocks) {
    hipLaunchKernelGGL(k_train_check_slots, dim3(nblocks), dim3(256), 0, s, data, nrec, want, first_bad);
}

// the eight launches of a step, each over all k members
void launch_group_trunk_fwd(hipStream_t s, int nb, int k, const Member* tab, const GroupStep& g, const NetOffsets& o, int net) {
    if (net == kNetLdp) hipLaunchKernelGGL(k_group_trunk_fwd<kNetLdp>, dim3(nb, k), dim3(256), 0, s, tab, g, o);
    else hipLaunchKernelGGL(k_group_trunk_fwd<kNetAi>, dim3(nb, k), dim3(256), 0, s, tab, g, o);
}
void launch_group_gemm(hipStream_t s, const GemmGroup* d_grps, int tiles_per, int k) {
    hipLaunchKernelGGL(k_group_gemm, dim3(tiles_per * k), dim3(256), 0, s, d_grps, tiles_per);
}
void launch_group_heads_fwd(hipStream_t s, int nb, int k, const Member* tab, const NetOffsets& o, uint64_t step, int net) {
    if (net == kNetLdp) hipLaunchKernelGGL(k_group_heads_fwd<kNetLdp>, dim3(nb, k), dim3(256), 0, s, tab, o, step);
    else hipLaunchKernelGGL(k_group_heads_fwd<kNetAi>, dim3(nb, k), dim3(256), 0, s, tab, o, step);
}
void launch_group_loss(hipStream_t s, int k, const Member* tab, int n, int with_grad) {
    hipLaunchKernelGGL(k_group_loss, dim3(k), dim3(256), 0, s, tab, n, with_grad);
}
void launch_group_heads_bwd(hipStream_t s, int nb, int k, const Member* tab, const NetOffsets& o) {
    hipLaunchKernelGGL(k_group_heads_bwd, dim3(nb, k), dim3(256), 0, s, tab, o);
}
void launch_group_trunk_bwd(hipStream_t s, int nb, int k, const Member* tab, const NetOffsets& o) {
    hipLaunchKernelGGL(k_group_trunk_bwd, dim3(nb, k), dim3(256), 0, s, tab, o);
}
void launch_group_update(hipStream_t s, int k, const Member* tab, int nb, const GroupRates& r, long n, const TuneMask& mask) {
    hipLaunchKernelGGL(k_group_update, dim3(1024, k), dim3(256), 0, s, tab, nb, r, n, mask);
}

}  // namespace train
}  // namespace ethcnn
