// ethcnn_train_util.h -- what the host sides of the ETH-CNN and the ETH-LSTM trainers share: error messages, the GEMM descriptor
// bookkeeping, the learning-rate schedule and the read-back of a step's loss / accuracy lists.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "ethcnn_ctx.h"
#include "ethcnn_train.h"

namespace ethcnn {
namespace train {

// the message of a failed call, printf-style, into *err; member >= 0: with the member of a trainer group named.  Returns code.
__attribute__((format(printf, 4, 5))) inline int fail(std::string* err, int member, int code, const char* fmt, ...) {
    char buf[640];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *err = member >= 0 ? "member " + std::to_string(member) + ": " + buf : std::string(buf);
    return code;
}
// terr(t, code, fmt, ...): t is a trainer or an engine (anything with an `err` string).  gerr(g, member, code, fmt, ...): g is an
// engine; the member is named when it serves a trainer group, not when it serves a solo trainer.  (Macros, so that the compiler
// checks the format against its arguments.)
#define terr(t, code, ...) ethcnn::train::fail(&(t)->err, -1, (code), __VA_ARGS__)
#define gerr(g, member, code, ...) ethcnn::train::fail(&(g)->err, (g)->group ? (member) : -1, (code), __VA_ARGS__)
#define TCHK(t, call)                                                                                           \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess) return terr((t), ETHCNN_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

inline void add_desc(GemmGroup& g, GemmDesc d) {
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

inline float lr_at(float lr_init, float decay_rate, int64_t decay_steps, int64_t step) {  // tf.train.exponential_decay(..., staircase=True)
    const double p = std::floor((double)step / (double)decay_steps);
    return (float)((double)lr_init * std::pow((double)decay_rate, p));
}

// the loss / accuracy lists of k members (stats[i]: member i's 8 device floats) into loss[3 k] / acc[3 k] (either may be NULL)
inline hipError_t read_stats(hipStream_t s, float* const* stats, int k, float* loss, float* acc) {
    float st[kMaxMembers][8];
    hipError_t e = hipSuccess;
    for (int i = 0; i < k && e == hipSuccess; ++i) e = hipMemcpyAsync(st[i], stats[i], sizeof st[i], hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    for (int i = 0; i < k && e == hipSuccess; ++i)
        for (int l = 0; l < 3; ++l) {
            if (loss) loss[3 * i + l] = st[i][l];
            if (acc) acc[3 * i + l] = st[i][3 + l];
        }
    return e;
}

}  // namespace train
}  // namespace ethcnn
