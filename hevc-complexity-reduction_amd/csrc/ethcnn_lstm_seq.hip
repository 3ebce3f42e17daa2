// ethcnn_lstm_seq.hip -- config #5 offline: the ETH-LSTM recurrence + LDP heads over a whole run of frames in ONE launch, and the
// gate post-pass.  The per-frame kernels (ethcnn_lstm.hip) are built for lock-step latency: every frame spreads its 28 hidden
// tiles over the whole chip and sends (c, h) -- 2 x 3.5 KB per CTU -- through HBM.  Offline all frames are known, the recurrence is
// sequential over frames and independent over CTUs, so here a block OWNS its 16-CTU column groups of one level for every frame:
//   block = 16 waves; level 16 (N = 256): one column group, wave t owns hidden tile t;
//                     level 32 (N = 128): two column groups x 8 tiles;  level 64 (N = 64): four column groups x 4 tiles.
//   A wave owns ALL FOUR gates (i, j, f, o) of its tile: four v_mfma_f32_16x16x4_f32 accumulators, each the canonical chain over
//   [x, h_prev] in k = 16 c + 4 g + e order (x chunks first, then h chunks), interleaved -- so the four pre-activations of hidden unit
//   u = 16 t + 4 g + r sit in slot r of the SAME lane and the cell update is lane-local; c stays in registers for the whole run.
//   h_new in C layout IS the B-operand quad of h chunk t of the next frame (and of fc2^T): it goes to LDS, double-buffered, and
//   nowhere else.  The kernel rows come from the packed image (kLstmPackOff) out of L2 every frame through a 3-chunk register ring
//   (2 MB at level 16: fits neither registers nor LDS).  Heads: wave j < N2/16 runs fc2^T tile j (operands from the packed fc2 image),
//   wave 0 of a column group fc3^T + sigmoid (W3 and b3 staged in LDS once per block); efs columns and the bias last -- the helpers
//   and the order of lstm_cell / lstm_heads.
// Per frame: three workgroup barriers, no flag, no spin-wait, no claim word, no atomic.  Bit-identical to the per-frame path.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ethcnn_canon_math.h"
#include "ethcnn_kernels.h"
#include "ethcnn_lstm_seq.h"
#include "ethcnn_spec.h"

namespace ethcnn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// The activation functions are the shared canonical ones (ethcnn_canon_math.h), the level tables (kLstmOff, LstmDims) those of
// ethcnn_spec.h, as in ethcnn_lstm.hip.

// what the body below works on: the block's row of the launch's table (SeqBatchRow), copied out of the kernel arguments.  Kept
// beside the row type because a body that reads the row in place compiles to other device code (another register allocation)
struct SeqParams {
    const float* vec;       // [F][n][448]
    const float* state_in;  // [n][2][448] or null
    float* state_out;       // [n][2][448]
    const float* blob;      // the LSTM bundle's payload + the packed images behind it
    float* probs;           // [F][n][21], ungated
    int n, F;
    int i_frame0;
    float efs0;             // qp / 51 * 0.18
};

constexpr int kSeqRing = 3;     // chunks of kernel rows in flight per wave (4 gates x dwordx4 each)
constexpr int kSeqWaves = 16;   // per block

template <int LV>
__device__ __forceinline__ void lstm_seq_level(const SeqParams& P, int blk, f32x4* smem) {
    using D = LstmDims<LV>;
    constexpr int N = D::N, N2 = D::N2, N3 = D::N3, O1 = D::O1, O3 = D::O3, NT = D::NT, NT2 = D::NT2, NC = 2 * NT;
    constexpr int SL = kSeqWaves / NT;  // column groups of the block
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int slot = wave / NT, t = wave % NT;
    const int col = lane & 15, g = lane >> 4;
    const int ctu_raw = (blk * SL + slot) * 16 + col;
    // a ragged group, or a column group behind the last one: computed on row n - 1 (with an in-place state possibly AFTER that row's
    // owner has stored its final state: harmless, the column is independent of every other one and is never stored)
    const bool valid = ctu_raw < P.n;
    const size_t row = (size_t)min(ctu_raw, P.n - 1);

    // LDS of one column group: [x quads: NT chunks][h quads, buffer 0: NT][h quads, buffer 1: NT] x 64 lanes; the B-operand quad of
    // lane (ctu, g) for chunk kc holds [x, h][16 kc + 4 g + 0..3] of that CTU.  The fc2 outputs (h2, NT2 <= NT quads) go to the h
    // buffer the chain has just finished with.
    f32x4* const xs = smem + slot * (3 * NT * 64);
    f32x4* const hb0 = xs + NT * 64;
    f32x4* const hb1 = hb0 + NT * 64;

    const float* const blob = P.blob;
    const float* const bk = blob + kLstmOff.v[LV][4];
    const float* const b2_0 = blob + kLstmOff.v[LV][0];
    const float* const W2_0 = blob + kLstmOff.v[LV][1];
    const float* const b3_0 = blob + kLstmOff.v[LV][2];
    const float* const W3_0 = blob + kLstmOff.v[LV][3];
    // gate q, chunk kc of tile t: one 1 KB run, a dwordx4 per lane (ethcnn_spec.h)
    // buffer loads: wave-uniform base + scalar offset of the (gate, chunk) run + lane * 16 -- no address registers per load (the runs lie
    // up to 128 KB apart, far beyond the immediate offset of a global load)
    const __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(blob) + kLstmBlobFloats + kLstmPackOff[LV] + (size_t)(t * 4 * NC) * 256, 0, 4 * NC * 1024, 0x00020000);
    const __amdgpu_buffer_rsrc_t rW2 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(blob) + kLstmBlobFloats + kLstmPackFc2Off[LV] + (size_t)(min(t, NT2 - 1) * NT) * 256, 0, NT * 1024, 0x00020000);
    const int voff = lane * 16;

    const int u0 = 16 * t + 4 * g;  // this lane's four hidden units: u0 + r
    float bias[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) bias[q][r] = bk[q * N + u0 + r];
    float cst[4] = {0.f, 0.f, 0.f, 0.f};
    f32x4 hlast = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (P.state_in) {
        const float4 cv = *reinterpret_cast<const float4*>(P.state_in + row * 2 * kNVec + O1 + u0);
        const float4 hv = *reinterpret_cast<const float4*>(P.state_in + row * 2 * kNVec + kNVec + O1 + u0);
        cst[0] = cv.x, cst[1] = cv.y, cst[2] = cv.z, cst[3] = cv.w;
        hlast = (f32x4){hv.x, hv.y, hv.z, hv.w};
    }
    hb0[t * 64 + lane] = hlast;
    // fc3 operands of the level (W3 with its efs rows, b3): staged once, shared by the block's column groups
    float* const sW3 = reinterpret_cast<float*>(smem + kSeqWaves * 3 * 64);
    float* const sB3 = sW3 + (N2 + 5) * N3;
    for (int i = threadIdx.x; i < (N2 + 5) * N3; i += 64 * kSeqWaves) sW3[i] = W3_0[i];
    if (threadIdx.x < N3) sB3[threadIdx.x] = b3_0[threadIdx.x];

    const float* const xsrc = P.vec + row * kNVec + O1 + u0;  // x chunk t of frame 0; a frame is n x 448 floats
    const size_t xstep = (size_t)P.n * kNVec;
    float4 xr = *reinterpret_cast<const float4*>(xsrc);
    int cur = 0;

#pragma unroll 1
    for (int f = 0; f < P.F; ++f) {
        // every weight address below is the same in every frame; left alone, the compiler hoists those loads out of the frame loop
        // (a thousand registers, spilled): an offset it cannot see through keeps each load in the frame that uses it
        int fz = 0;
        asm volatile("" : "+s"(fz));
        const float* const b2 = b2_0 + fz;
        const float* const W2 = W2_0 + fz;
        xs[t * 64 + lane] = (f32x4){xr.x, xr.y, xr.z, xr.w};
        if (f + 1 < P.F) xr = *reinterpret_cast<const float4*>(xsrc + (size_t)(f + 1) * xstep);  // lands under this frame's chain
        f32x4 ring[kSeqRing][4];
#pragma unroll
        for (int d = 0; d < kSeqRing; ++d)
#pragma unroll
            for (int q = 0; q < 4; ++q) ring[d][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rK, voff, fz + (q * NC + d) * 1024, 0));
        __syncthreads();  // x of this frame and h of the previous one are staged
        const f32x4* const hcur = cur ? hb1 : hb0;
        f32x4* const hnew = cur ? hb0 : hb1;
        f32x4* const h2T = cur ? hb1 : hb0;  // (free once the barrier behind the cell update has been passed)

        f32x4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < NC; ++kc) {
            const int sl = kc % kSeqRing;
            const f32x4 hq = (kc < NT) ? xs[kc * 64 + lane] : hcur[(kc - NT) * 64 + lane];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[q] = MFMA16(ring[sl][q][e], hq[e], acc[q]);
                }
            if (kc + kSeqRing < NC) {
#pragma unroll
                for (int q = 0; q < 4; ++q) ring[sl][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rK, voff, fz + (q * NC + kc + kSeqRing) * 1024, 0));
            }
            __builtin_amdgcn_sched_barrier(0);  // (the order above is the schedule: every load a ring's depth ahead of its use)
        }


        // cell update, lane-local: LSTMCell(forget_bias = 1, cell_clip = 5)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float gi = acc[0][r] + bias[0][r], gj = acc[1][r] + bias[1][r], gf = acc[2][r] + bias[2][r], go = acc[3][r] + bias[3][r];
            float cc = canon_sigmoid(gf + 1.0f) * cst[r] + canon_sigmoid(gi) * canon_tanh(gj);
            cc = fminf(fmaxf(cc, -5.0f), 5.0f);
            cst[r] = cc;
            hlast[r] = canon_sigmoid(go) * canon_tanh(cc);
        }
        hnew[t * 64 + lane] = hlast;

        const float efs[5] = {P.efs0, 0.0f, 0.0f, 0.0f, 0.0f};
        const int phase = (P.i_frame0 + f) & 3;
        // the fc2 operands of this wave's tile are requested here, in front of the barrier (behind the cell update: beside its
        // temporaries they do not fit the 128 registers of a 16-wave block)
        __builtin_amdgcn_sched_barrier(0);
        f32x4 w2a[NT];
        if (t < NT2) {
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) w2a[tt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rW2, voff, fz + tt * 1024, 0));
        }
        __syncthreads();  // h_new of every tile is in LDS; nobody reads x or the old h any more

        // ---- heads: fc2^T tile t by wave t < NT2 (step (tt, r) consumes k = 16 tt + 4 g + r), then fc3^T by wave 0 of the group
        if (t < NT2) {
            f32x4 a2 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) {
                const f32x4 hv = hnew[tt * 64 + lane];
#pragma unroll
                for (int r = 0; r < 4; ++r) a2 = MFMA16(w2a[tt][r], hv[r], a2);
            }
            float we[4][5], b2v[4];  // the efs rows + bias of this lane's four outputs
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int e = 0; e < 5; ++e) we[r][e] = W2[(N + e) * N2 + 16 * t + 4 * g + r];
                b2v[r] = b2[16 * t + 4 * g + r];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = a2[r];
#pragma unroll
                for (int e = 0; e < 5; ++e) v = fmaf(e == 0 ? efs[0] : (e - 1 == phase ? 1.0f : 0.0f), we[r][e], v);
                a2[r] = canon_lrelu(v + b2v[r]);
            }
            h2T[t * 64 + lane] = a2;
        }
        __syncthreads();  // h2 of every fc2 tile is in LDS
        if (t == 0) {
            f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
            const int c3 = min(col, N3 - 1);  // (columns >= N3 feed zeros: read from a valid address, then dropped)
#pragma unroll
            for (int j = 0; j < NT2; ++j) {
                const f32x4 hv = h2T[j * 64 + lane];
#pragma unroll
                for (int r = 0; r < 4; ++r) z = MFMA16(col < N3 ? sW3[(16 * j + 4 * g + r) * N3 + c3] : 0.0f, hv[r], z);
            }
            float* const out = P.probs + ((size_t)f * P.n + row) * kNOut + O3;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = 4 * g + r;
                if (o < N3 && valid) {
                    float zz = z[r];
#pragma unroll
                    for (int e = 0; e < 5; ++e) zz = fmaf(e == 0 ? efs[0] : (e - 1 == phase ? 1.0f : 0.0f), sW3[(N2 + e) * N3 + o], zz);
                    out[o] = canon_sigmoid(zz + sB3[o]);
                }
            }
        }
        cur ^= 1;
        // (the next frame writes x, which nobody reads behind the second barrier, and -- behind its own first barrier, which wave 0
        // reaches only after fc3 -- the h buffer that holds h2)
    }

    if (valid) {  // the state after the last frame, once
        float* const so = P.state_out + row * 2 * kNVec + O1 + u0;
        *reinterpret_cast<float4*>(so) = make_float4(cst[0], cst[1], cst[2], cst[3]);
        *reinterpret_cast<float4*>(so + kNVec) = make_float4(hlast[0], hlast[1], hlast[2], hlast[3]);
    }
}

// ONE kernel for every form of the call.  Up to 32 independent sequences in one launch; a row of the table is a sequence with its own
// n, F and i_frame0, and the solo and group calls are the uniform case: K rows with the same three.  The kernel only chooses whose
// row a block works on and calls the body above.  The block -> (level, row, block of the row) mapping comes from one prefix array per
// level over the rows' block counts (ethcnn_lstm_seq.h::lstm_seq_blocks).  Linear, level-major grid, level 16 first (the long chains
// first); inside a level the rows stand in the order of the table, which the launcher sorts by frames of this launch,
// most first: a block lasts as long as its row has frames, so the long ones are dispatched first.  A block finds its row by a scan of
// the level's prefix sums -- block-uniform, scalar loads from the kernel arguments (2448 bytes: 32 rows of 64, 3 x 33 ints) -- and
// then runs the same body with the row's own n.  No block waits for another one; which block computes what is fixed by the table.
struct SeqBatchParams {
    SeqBatchRow r[kLstmSeqBatchMax];
    int pre[3][kLstmSeqBatchMax + 1];  // [level 16, 32, 64][row]: blocks of the rows in front of it; [k]: the level's total
    int k;
};
static_assert(sizeof(SeqBatchRow) == 64 && sizeof(SeqBatchParams) <= 4096, "the table travels in the kernel arguments");

__global__ __launch_bounds__(1024) void k_lstm_seq_batch(SeqBatchParams B) {
    __shared__ f32x4 smem[kSeqWaves * 3 * 64 + ((192 + 5) * 16 + 16) / 4];  // 48 KB of quads + the fc3 operands (12.4 KB at level 16)
    const int K = B.k, n2 = B.pre[0][K], n1 = B.pre[1][K];
    const int b = (int)blockIdx.x;
    const int lv = b < n2 ? 0 : (b < n2 + n1 ? 1 : 2);
    const int r = b < n2 ? b : (b < n2 + n1 ? b - n2 : b - n2 - n1);  // position inside the level
    int j = 0;
    while (j + 1 < K && B.pre[lv][j + 1] <= r) ++j;
    const int blk = r - B.pre[lv][j];
    const SeqBatchRow& R = B.r[j];
    SeqParams P;
    P.vec = R.vec;
    P.state_in = R.state_in;
    P.state_out = R.state_out;
    P.blob = R.blob;
    P.probs = R.probs;
    P.n = R.n;
    P.F = R.F;
    P.i_frame0 = R.i_frame0;
    P.efs0 = R.efs0;
    if (lv == 0) lstm_seq_level<2>(P, blk, smem);
    else if (lv == 1) lstm_seq_level<1>(P, blk, smem);
    else lstm_seq_level<0>(P, blk, smem);
}

void launch_lstm_seq_batch(const SeqBatchRow* rows, int k, hipStream_t s) {
    SeqBatchParams B;
    int order[kLstmSeqBatchMax];
    for (int j = 0; j < k; ++j) order[j] = j;
    std::stable_sort(order, order + k, [&](int a, int b) { return rows[a].F > rows[b].F; });
    for (int j = 0; j < kLstmSeqBatchMax; ++j) B.r[j] = rows[order[j < k ? j : 0]];
    for (int lv = 0; lv < 3; ++lv) {
        int at = 0;
        for (int j = 0; j <= kLstmSeqBatchMax; ++j) {
            B.pre[lv][j] = at;
            if (j < k) {
                int64_t blocks[3];
                lstm_seq_blocks(B.r[j].n, blocks);
                at += (int)blocks[lv];
            }
        }
    }
    B.k = k;
    const unsigned blocks = (unsigned)(B.pre[0][k] + B.pre[1][k] + B.pre[2][k]);
    hipLaunchKernelGGL(k_lstm_seq_batch, dim3(blocks), dim3(64 * kSeqWaves), 0, s, B);
}

// ---- gates: the tf.cond pair of net():305,317 per (frame, mini-batch of 1024 CTUs).  One block owns the mini-batch: it reduces the
// two predicates over the UNGATED probabilities (any y64 > thr1; any y32 > thr2) and zero-fills what the per-frame launch's last
// block zero-fills: y32 and y16 when the first gate is closed, y16 when the second is -- which, behind a closed first gate, sees
// zeros and is open only if 0 > thr2.
__device__ __forceinline__ void lstm_seq_gates_body(float* __restrict__ probs, int n, int chunks, float thr1, float thr2) {
    const int frame = (int)blockIdx.x / chunks, c0 = ((int)blockIdx.x - frame * chunks) * kSubBatch, cnt = min(n - c0, kSubBatch);
    float* const p = probs + ((size_t)frame * n + c0) * kNOut;
    int a32 = 0, a16 = 0;
    for (int i = threadIdx.x; i < cnt; i += (int)blockDim.x) {
        const float* q = p + (size_t)i * kNOut;
        a32 |= (q[0] > thr1) ? 1 : 0;
        a16 |= (q[1] > thr2 || q[2] > thr2 || q[3] > thr2 || q[4] > thr2) ? 1 : 0;
    }
    const bool open32 = __syncthreads_or(a32) != 0;
    const bool any16 = __syncthreads_or(a16) != 0;
    const bool open16 = open32 ? any16 : (0.0f > thr2);
    if (open32 && open16) return;
    for (int idx = threadIdx.x; idx < cnt * kNOut; idx += (int)blockDim.x) {
        const int j = idx % kNOut;
        if (j != 0 && (j < 5 ? !open32 : !open16)) p[idx] = 0.0f;
    }
}

// grid (max over rows of frames x mini-batches, rows); a block behind its row's last (frame, mini-batch) returns at once.  Every row
// has a threshold pair of its own: like n and F it is read by the block-uniform row index, a scalar load from the kernel-argument
// segment (768 bytes), so no lane indexes the table and nothing of it lives in scratch.
struct SeqGateBatch {
    float* probs[kLstmSeqBatchMax];
    int n[kLstmSeqBatchMax], F[kLstmSeqBatchMax];
    float thr1[kLstmSeqBatchMax], thr2[kLstmSeqBatchMax];
};
static_assert(sizeof(SeqGateBatch) == 768, "the gate launch's kernel arguments");
__global__ __launch_bounds__(256) void k_lstm_seq_gates_batch(SeqGateBatch Q) {
    const int n = Q.n[blockIdx.y], chunks = (n + kSubBatch - 1) / kSubBatch;
    if ((int)blockIdx.x >= chunks * Q.F[blockIdx.y]) return;
    lstm_seq_gates_body(Q.probs[blockIdx.y], n, chunks, Q.thr1[blockIdx.y], Q.thr2[blockIdx.y]);
}

void launch_lstm_seq_gates_batch(const SeqBatchRow* rows, int k, const float* thr1, const float* thr2, hipStream_t s) {
    SeqGateBatch Q;
    unsigned gx = 1;
    for (int j = 0; j < kLstmSeqBatchMax; ++j) {
        const int r = j < k ? j : 0;
        const SeqBatchRow& R = rows[r];
        Q.probs[j] = R.probs, Q.n[j] = R.n, Q.F[j] = R.F, Q.thr1[j] = thr1[r], Q.thr2[j] = thr2[r];
        gx = std::max(gx, (unsigned)((R.n + kSubBatch - 1) / kSubBatch) * (unsigned)R.F);
    }
    hipLaunchKernelGGL(k_lstm_seq_gates_batch, dim3(gx, (unsigned)k), dim3(256), 0, s, Q);
}

void launch_lstm_seq_gates_batch(const SeqBatchRow* rows, int k, float thr1, float thr2, hipStream_t s) {
    float t1[kLstmSeqBatchMax], t2[kLstmSeqBatchMax];
    for (int j = 0; j < k; ++j) t1[j] = thr1, t2[j] = thr2;
    launch_lstm_seq_gates_batch(rows, k, t1, t2, s);
}

}  // namespace ethcnn
