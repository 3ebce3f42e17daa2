// ethcnn_canon_math.h -- the canonical activation functions of the exact path: ONE device copy of
// lrelu / exp / sigmoid / tanh for the ETH-CNN heads (ethcnn_heads_pass.h, ethcnn_heads_fast.hip) and the ETH-LSTM kernels
// (ethcnn_lstm.hip, ethcnn_lstm_seq.hip).  The operation sequence is the contract with the oracle (oracle/ethcnn_oracle.c:
// lrelu, oracle_expf, sigmoidf, tanhf_c): the same fmaf / mul / rint / exponent arithmetic, in the same order, so that every
// float -- subnormal, saturated, infinite or NaN -- gives the oracle's bits.
//
// Non-finite arguments follow TensorFlow (sigmoid, tanh and exp of NaN are NaN; the reference's graphs have no clamp of their
// own): the clamps below are COMPARISONS, which a NaN fails, not fminf / fmaxf, which return the other operand and turned a
// NaN pre-activation into an ordinary-looking 1.8e-35 (sigmoid) or 1 (tanh).  +Inf clamps to 80, -Inf to -86.
// tests/test_gpu_edge_values.py compares every path that includes this header with the oracle at those values.
#pragma once
#include <hip/hip_runtime.h>

namespace ethcnn {

// tf.nn.leaky_relu, alpha 0.2, emitted as Maximum(alpha * x, x) (net_CNN.py:69); both operands are NaN when h is
__device__ __forceinline__ float canon_lrelu(float h) { return fmaxf(0.2f * h, h); }

__device__ __forceinline__ float canon_exp(float x) {
    x = (x > 80.0f) ? 80.0f : x;  // keeps 2^n * p normal; a NaN passes both comparisons unchanged
    x = (x < -86.0f) ? -86.0f : x;
    if (x != x) return x;  // before the float -> int conversion below, which is undefined for a NaN
    const float n = rintf(x * 1.44269504088896341f);
    float r = fmaf(n, -0.693145751953125f, x);
    r = fmaf(n, -1.42860682030941723212e-6f, r);
    float p = 1.0f / 5040.0f;
    p = fmaf(p, r, 1.0f / 720.0f);
    p = fmaf(p, r, 1.0f / 120.0f);
    p = fmaf(p, r, 1.0f / 24.0f);
    p = fmaf(p, r, 1.0f / 6.0f);
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    return __int_as_float(__float_as_int(p) + (((int)n) << 23));
}

__device__ __forceinline__ float canon_sigmoid(float z) { return 1.0f / (1.0f + canon_exp(-z)); }

__device__ __forceinline__ float canon_tanh(float x) {
    const float e = canon_exp(2.0f * x);
    return (e - 1.0f) / (e + 1.0f);
}

}  // namespace ethcnn
