// ethcnn_decide.cpp -- host side of the partition decisions (include/ethcnn.h "partition decisions"): the entries around the kernel of
// ethcnn_decide.hip over a simulator's set, and the host-only counters of a slice of codes.
#include "ethcnn_analysis.h"
#include "ethcnn_decide.h"

using namespace ethcnn::decide;
using ethcnn::sim::kStageCtus;

namespace {
// everything of a call that does not depend on the layout: 0, or ETHCNN_ERR_ARG with the message set
int check_call(ethcnn_sim* k, const ethcnn_sim_thr* thr, int gate_order, int mid_k, Cand* cand) {
    ethcnn_ctx* c = k->c;
    if (!thr) return set_err(c, ETHCNN_ERR_ARG, "null candidate");
    if (int rc = ethcnn::sim::check_cand(c, *thr, 0)) return rc;
    if (int rc = ethcnn::sim::check_gates(c, gate_order)) return rc;
    if (mid_k < 0 || mid_k > 1024) return set_err(c, ETHCNN_ERR_ARG, "mid_k = %d outside 0..1024", mid_k);
    for (int l = 0; l < 3; ++l) cand->up[l] = thr->up_k[l], cand->down[l] = thr->down_k[l];
    cand->gate_order = gate_order;
    cand->mid = mid_k;
    return 0;
}

int check_window(ethcnn_sim* k, int64_t first, int64_t n) {
    if (first < 0 || n < 0 || first > k->ctus || n > k->ctus - first)
        return set_err(k->c, ETHCNN_ERR_ARG, "CTUs %lld .. %lld + %lld lie outside the set of %lld", (long long)first, (long long)first, (long long)n,
                       (long long)k->ctus);
    return 0;
}

// launch + wait; the outputs are device pointers indexed from CTU `first`
int run(ethcnn_sim* k, const Cand& cand, int64_t first, int64_t n, const Planes& pl, uint8_t* d_codes, uint8_t* d_reach, uint8_t* d_depth) {
    ethcnn_ctx* c = k->c;
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;  // the context's completion word does not cover this launch
    launch_decide(c->stream, k->d_recs + first * ethcnn::sim::kRecDwords, k->d_m, (long)n, cand, pl, d_codes, d_reach, d_depth);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
}  // namespace

extern "C" int ethcnn_decide_device(ethcnn_sim* k, const ethcnn_sim_thr* thr, int gate_order, int mid_k, int64_t first, int64_t n, uint8_t* d_codes,
                                    uint8_t* d_reach, uint8_t* d_depth) {
    if (!k) return ETHCNN_ERR_ARG;
    Cand cand;
    if (int rc = check_call(k, thr, gate_order, mid_k, &cand)) return rc;
    if (int rc = check_window(k, first, n)) return rc;
    if (((uintptr_t)d_codes | (uintptr_t)d_reach | (uintptr_t)d_depth) % 4) return set_err(k->c, ETHCNN_ERR_ARG, "device buffer not 4-byte aligned");
    if (n == 0) return ETHCNN_OK;
    return run(k, cand, first, n, Planes{nullptr, 0, 0, 0, 0}, d_codes, d_reach, d_depth);
}

extern "C" int ethcnn_decide_set_piece(ethcnn_sim* k, int64_t ctus) {
    if (!k) return ETHCNN_ERR_ARG;
    if (ctus < 0) return set_err(k->c, ETHCNN_ERR_ARG, "negative piece size %lld", (long long)ctus);
    k->decide_piece = ctus;
    return ETHCNN_OK;
}

extern "C" int ethcnn_decide(ethcnn_sim* k, const ethcnn_sim_thr* thr, int gate_order, int mid_k, int64_t first, int64_t n, uint8_t* codes, uint8_t* reach,
                             uint8_t* depth) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    Cand cand;
    if (int rc = check_call(k, thr, gate_order, mid_k, &cand)) return rc;
    if (int rc = check_window(k, first, n)) return rc;
    const int64_t per = (codes ? kCodeBytes : 0) + (reach ? kBlockBytes : 0) + (depth ? kBlockBytes : 0);
    if (n == 0 || per == 0) return ETHCNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t piece = std::min(n, k->decide_piece > 0 ? k->decide_piece : kStageCtus);
    // a piece's outputs side by side in one buffer (each part a multiple of 16 bytes long but for the codes, which come last)
    Scratch d;
    if (int rc = d.alloc(c, (size_t)(piece * per), "partition decisions", true)) return rc;
    uint8_t* d_reach = reach ? d.at() : nullptr;
    uint8_t* d_depth = depth ? d.at(reach ? piece * kBlockBytes : 0) : nullptr;
    uint8_t* d_codes = codes ? d.at(piece * (per - kCodeBytes)) : nullptr;
    int rc = 0;
    for (int64_t at = 0; at < n && !rc; at += piece) {
        const int64_t cur = std::min(piece, n - at);
        rc = run(k, cand, first + at, cur, Planes{nullptr, 0, 0, 0, 0}, d_codes, d_reach, d_depth);
        hipError_t e = hipSuccess;
        if (!rc && codes) e = hipMemcpyAsync(codes + at * kCodeBytes, d_codes, (size_t)(cur * kCodeBytes), hipMemcpyDeviceToHost, c->stream);
        if (!rc && e == hipSuccess && reach) e = hipMemcpyAsync(reach + at * kBlockBytes, d_reach, (size_t)(cur * kBlockBytes), hipMemcpyDeviceToHost, c->stream);
        if (!rc && e == hipSuccess && depth) e = hipMemcpyAsync(depth + at * kBlockBytes, d_depth, (size_t)(cur * kBlockBytes), hipMemcpyDeviceToHost, c->stream);
        if (!rc && e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (!rc && e != hipSuccess) {
            (void)hipGetLastError();
            rc = set_err(c, ETHCNN_ERR_DEVICE, "partition decisions: %s", hipGetErrorString(e));
        }
    }
    return rc;
}

extern "C" int ethcnn_decide_frames_device(ethcnn_sim* k, const ethcnn_sim_thr* thr, int gate_order, int mid_k, int64_t first, int width, int height,
                                           int64_t nframes, uint8_t* d_codes, uint8_t* d_reach, uint8_t* d_planes) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    Cand cand;
    if (int rc = check_call(k, thr, gate_order, mid_k, &cand)) return rc;
    ethcnn::sim::PicSize s;
    if (int rc = ethcnn::sim::check_size(c, width, height, 8, &s)) return rc;
    if (d_planes && (width % 16 || height % 16))
        return set_err(c, ETHCNN_ERR_ARG, "label planes exist for sizes that are multiples of 16: got %d x %d", width, height);
    if (first < 0 || nframes < 0) return set_err(c, ETHCNN_ERR_ARG, "negative first CTU or frame count");
    if (((uintptr_t)d_codes | (uintptr_t)d_reach) % 4) return set_err(c, ETHCNN_ERR_ARG, "device buffer not 4-byte aligned");
    if (int rc = ethcnn::sim::check_frame_run(k, first, width, height, nframes)) return rc;
    if (nframes == 0) return ETHCNN_OK;
    return run(k, cand, first, nframes * s.ctus(), Planes{d_planes, s.ctus_w, s.ctus_h, s.w16, s.h16}, d_codes, d_reach, nullptr);
}

extern "C" int ethcnn_decide_counts_from_codes(const uint8_t* codes, int64_t n, ethcnn_sim_counts* counts_out) {
    if (!counts_out || n < 0 || (n && !codes)) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_decide_counts_from_codes: null argument or negative count");
    ethcnn_sim_counts s;
    std::memset(&s, 0, sizeof s);
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t* q = codes + i * kCodeBytes;
        for (int r = 0; r < 21; ++r) {
            const int l = r == 0 ? 0 : r < 5 ? 1 : 2, code = q[r] & 7, wrong = q[r] & 8;
            if (q[r] > 15 || code > 4 || (wrong && code != 1 && code != 2))
                return set_err(nullptr, ETHCNN_ERR_FORMAT, "ethcnn_decide_counts_from_codes: CTU %lld, node %d holds %d, which is no code", (long long)i, r, q[r]);
            s.checked[l] += code & 1;
            s.split_only[l] += code == 2;
            s.current_only[l] += code == 1;
            s.both[l] += code == 3;
            s.edge_split[l] += code == 4;
            s.wrong_split[l] += wrong && code == 2;
            s.wrong_stop[l] += wrong && code == 1;
        }
        if (q[21] > 31 || q[22] > 64 || q[23])
            return set_err(nullptr, ETHCNN_ERR_FORMAT, "ethcnn_decide_counts_from_codes: CTU %lld: bytes 21..23 = %d %d %d are no flags / 8 x 8 count / zero",
                           (long long)i, q[21], q[22], q[23]);
        s.checked[3] += q[22];
        s.bad_ctus += q[21] & 1;
    }
    *counts_out = s;
    return ETHCNN_OK;
}
