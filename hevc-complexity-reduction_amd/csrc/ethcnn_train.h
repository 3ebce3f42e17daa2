// ethcnn_train.h -- shared between the training kernels (ethcnn_train_kernels.hip) and their host side (ethcnn_train.cpp: a trainer's
// state; ethcnn_train_group.cpp: the step engine behind the solo and the group entry points).
//
// There is ONE step path.  It trains K >= 1 models ("members") of one net, batch and tuning mode at once; a solo trainer is the
// case K = 1.  One training step of ETH-CNN (All-Intra; ETH-CNN_Training_AI/net_CTU64.py:94-196) at batch B is 8 launches on the
// context's stream, each over all K members, in this order (grids: "the member table" below):
//   1 k_group_trunk_fwd   one block per sample: draw / read the sample index and QP, 4096 luma bytes -> the three pooled, mean-removed
//                         branch images, conv1..3 + leaky-ReLU; keeps images and conv1 outputs (per-sample trunk record) and writes the
//                         2688 features (+ a ones column) = F_aug [B][2689]
//   2 k_group_gemm        FC1 forward: F [B,2688] x W1 [2688,448] (the three heads' tensors as three descriptors), MFMA 32x32x2 f32
//   3 k_group_heads_fwd   one block per sample: FC1 bias + leaky + dropout, FC2 / FC3 of the three heads, sigmoid
//   4 k_group_loss        one block per member: the batch-global label counts, the loss / accuracy lists, dL/dlogit per sample
//   5 k_group_heads_bwd   one block per sample: dlogit -> dZ2 -> dZ1 (through the dropout masks and the leaky-ReLUs)
//   6 k_group_gemm        one grouped launch: dF = dZ1 x W1^T (K split over the three heads' tensors) and the nine FC weight / bias
//                         gradients X_aug^T x dZ (bias = the ones row), written in blob layout
//   7 k_group_trunk_bwd   one block per sample: dF -> the 18 conv tensors' per-sample gradient partials
//   8 k_group_update      every parameter: conv gradients summed over the batch in sample order, then the momentum update
// Low-Delay-P residual net (ETH-CNN_Training_LDP/net_CTU64.py:94-209): the same chain, with launches 1 and 3 instantiated for kNetLdp
// (16516-byte records, the sample's slot, residual scaling, the 0.18 QP feature).  With a tuning mode 1..3 (PARTLY_TUNING_MODE: only
// one head's six FC tensors are optimised) the conv gradients have no reader, so a step is 7 launches: launch 6 holds only the tuned
// head's three weight / bias GEMMs (no dF = dZ1 W1^T), launch 7 (trunk backward) is skipped, and launch 8 leaves every other tensor
// and its accumulator untouched.
// Determinism: no atomics; every sum has one owner thread and a fixed order (MFMA chains run k in order), so the same inputs give the
// same bits on every run.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

namespace ethcnn {
namespace train {

constexpr int kRec = 4992;        // bytes per training record (input_data.py:16): 4096 luma, 64 pad, 52 x 16 label bytes
constexpr int kLabelBase = 4160;  // label row of QP q at kLabelBase + 16 q (input_data.py:104)
constexpr int kRecLdp = 16516;    // LDP record (input_data.py:48-50): 64 header bytes, then 4 slots of [qp | 16 labels | 4096 residual]
constexpr int kSlotBase = 64, kSlotBytes = 4113;
enum { kNetAi = 0, kNetLdp = 1 };  // ETHCNN_TRAIN_NET_AI / _LDP
constexpr int kTF = 2688, kLdF = 2689, kTV = 448, kT2 = 336, kTOut = 21;
constexpr int kConvFloats = 14808;  // the 18 conv tensors lie at blob floats [0, 14808) (sorted keys "Variable*")
constexpr int kTrunkRec = 10752;    // per-sample trunk record: images S 4096 | M 1024 | L 256, conv1 S 4096 | M 1024 | L 256
constexpr int kMaxGemm = 12;

// counter-based RNG (documented in include/ethcnn.h, regenerated in numpy by the tests)
__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t draw(uint64_t seed, uint64_t stream, uint64_t step, uint64_t slot, uint64_t unit) {
    return mix64(mix64(mix64(seed ^ (stream * 0xD1B54A32D192ED03ull)) ^ step) ^ ((slot << 12) | unit));
}
enum { kStreamIndex = 1, kStreamQp = 2, kStreamDropout = 3 };

// A pointer that a kernel reads from a table in memory is a generic pointer to the compiler, which then emits FLAT accesses; a pointer
// that arrives as a kernel argument is known to be device memory.  The member tables hold device-memory pointers only: saying so
// gives the global_load / global_store a by-value argument would get.  field: a pointer member of a table entry IN MEMORY; it is
// loaded as a global-address-space pointer (same 64 bits) and only then converted, which is how the compiler treats kernel arguments.
template <class T>
__device__ __forceinline__ T* as_global(T* const& field) {
    __attribute__((address_space(1))) T* p;
    __builtin_memcpy(&p, &field, sizeof p);  // the same 64 bits, read as a global pointer: no lvalue of another type
    return (T*)p;
}

// C[m][n] = sum_k A(m,k) B(k,n); A(m,k) = A[m sam + k sak]; B(k,n) = Bs[s][(k - kseg[s]) sbk[s] + n sbn[s]] for the last segment s with
// kseg[s] <= k (segment starts are multiples of 32); rows m < msplit go to C[m ldc + n], rows m >= msplit to C2[(m - msplit) ldc + n].
struct GemmDesc {
    int M, N, K, nseg;
    const float* A;
    long sam, sak;
    const float* B[3];
    long sbk[3], sbn[3];
    int kseg[3];
    float* C;
    float* C2;
    long ldc;
    int msplit, tiles_n, tile_begin;
};
struct GemmGroup {
    GemmDesc d[kMaxGemm];
    int n, tiles;
};

// blob float offsets of the tensors the kernels touch (from kTensors, filled on the host)
struct NetOffsets {
    int convw[3][3], convb[3][3];  // [branch S, M, L][layer 1..3]
    int w1[3], b1[3], w2[3], b2[3], w3[3], b3[3];  // heads 64, 32, 16
};

// the parameter ranges [lo, hi) (blob floats) the update optimises; n == 0: all of them
struct TuneMask {
    long lo[6], hi[6];
    int n;
};

// ---- the member table (include/ethcnn.h "training" and "training, several models at once"): K >= 1 independent trainers of one
// net, batch and tuning mode in every launch of a step.  Launch i of the 8 (tune 1..3: 7) above covers all K members:
//   trunk forward / heads forward / heads backward / trunk backward   grid (B, K): block (b, m) is sample slot b of member m
//   loss                                                              K blocks: block m owns member m's batch-global counts
//   GEMM                                                              K x T blocks, T = the tiles of one member's descriptor group:
//                                                                     block i runs tile i % T of member i / T (every member has the
//                                                                     same shapes); the members' GemmGroups lie side by side
//   update                                                            grid (1024, K): row m strides over member m's parameters
// The member is the grid's last dimension, so what a body sees in blockIdx.x and gridDim.x does not depend on K or m; no sum crosses
// members and nothing is atomic.  There is no other path, so member m computes the same bits whatever K and m are, a solo trainer
// (K = 1) included.  The members share the sample records and nothing else.
// The table lives in device memory and changes only when a member's QP list does (set_qps, and an LDP training-set upload, which
// resets it to the four slot QPs); the host marks it stale then and uploads it again before the next step, after waiting for the
// steps in flight.  What changes from launch to launch goes by value: the step number, the sample set (GroupStep) and the K learning
// rates of the step (GroupRates).  An evaluation works on tables of its own (one per piece), never on the step table.
struct Member {
    float *W, *acc, *grad;                // blob layout: weights, momentum accumulators, gradient
    const int32_t *idx_in, *qp_in;        // explicit batch / evaluation samples (ignored when GroupStep.drawn)
    int32_t *idx, *qp;                    // the batch's sample indices and QPs, as drawn or read
    float *lab, *trunk, *F, *Z1, *A1, *M1, *H1, *A2, *M2, *H2, *P, *dZ3, *dZ2, *dZ1, *dF, *part, *stats;  // workspaces
    uint64_t seed;
    int qps[52];
    int nqps;
    int qp_fixed;  // >= 0: every sample at this QP (evaluation)
    int dropout;
    float momentum;
};
struct GroupStep {
    const uint8_t* data;  // the shared records
    long nrec;
    int slot_of_qp[52];  // LDP: the record slot holding QP q (the set's four slot QPs; -1 elsewhere)
    uint64_t step;
    int drawn;  // 1: indices and QPs drawn on the device
};
constexpr int kMaxMembers = 8;
struct GroupRates {
    float lr[kMaxMembers];
};

// launchers (ethcnn_train_kernels.hip), each over all k members; the ETH-LSTM engine uses the GEMM and the loss unchanged
void launch_group_trunk_fwd(hipStream_t s, int nb, int k, const Member* tab, const GroupStep& g, const NetOffsets& o, int net);
void launch_group_gemm(hipStream_t s, const GemmGroup* d_grps, int tiles_per, int k);
void launch_group_heads_fwd(hipStream_t s, int nb, int k, const Member* tab, const NetOffsets& o, uint64_t step, int net);
void launch_group_loss(hipStream_t s, int k, const Member* tab, int n, int with_grad);
void launch_group_heads_bwd(hipStream_t s, int nb, int k, const Member* tab, const NetOffsets& o);
void launch_group_trunk_bwd(hipStream_t s, int nb, int k, const Member* tab, const NetOffsets& o);
void launch_group_update(hipStream_t s, int k, const Member* tab, int nb, const GroupRates& r, long n, const TuneMask& mask);
void launch_check_slots(hipStream_t s, const uint8_t* data, long nrec, uint32_t want, long* first_bad, int nblocks);

}  // namespace train
}  // namespace ethcnn
