// ethcnn_budget.cpp -- host side of the search budget (include/ethcnn.h "search budget"): the entries around the two kernels of
// ethcnn_budget.hip over a simulator's set, and the host-only ladder, companion thresholds and per-frame choice.
#include "ethcnn_analysis.h"
#include "ethcnn_budget.h"

using namespace ethcnn::budget;
using ethcnn::sim::kStageCtus;

namespace {
int check_ladder(ethcnn_ctx* c, const ethcnn_sim_thr* ladder, int64_t K) {
    if (!ladder) return set_err(c, ETHCNN_ERR_ARG, "null ladder");
    if (int rc = sim::check_rung_count(c, K)) return rc;
    for (int64_t i = 0; i < K; ++i)
        if (int rc = sim::check_cand(c, ladder[i], (long long)i)) return rc;
    return 0;
}

// the window of whole frames; *per = CTUs a frame
int check_window(ethcnn_sim* k, int64_t first, int width, int height, int64_t nframes, int64_t* per) {
    ethcnn_ctx* c = k->c;
    sim::PicSize s;
    if (int rc = sim::check_size(c, width, height, 8, &s)) return rc;
    if (first < 0 || nframes < 0) return set_err(c, ETHCNN_ERR_ARG, "negative first CTU or frame count");
    *per = s.ctus();
    if (*per >= kMaxFrameCtus) return set_err(c, ETHCNN_ERR_ARG, "a frame of %lld CTUs does not count in 32 bits (fewer than 2^24)", (long long)*per);
    return ethcnn::sim::check_frame_run(k, first, width, height, nframes);
}

// rows of six ints (up_k[3], down_k[3]) into the set's device table `which`
int upload_thr(ethcnn_sim* k, int which, const std::vector<int>& rows) {
    ethcnn_ctx* c = k->c;
    const int64_t n = (int64_t)rows.size() / 6;
    if (n > k->cap_budget_thr[which]) {
        int* p = nullptr;
        if (hipMalloc((void**)&p, (size_t)n * 24) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(c, ETHCNN_ERR_NOMEM, "search budget: %lld bytes of thresholds do not fit in device memory", (long long)(n * 24));
        }
        if (k->d_budget_thr[which]) (void)hipFree(k->d_budget_thr[which]);
        k->d_budget_thr[which] = p;
        k->cap_budget_thr[which] = n;
    }
    HIPCHK(c, hipMemcpyAsync(k->d_budget_thr[which], rows.data(), (size_t)n * 24, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (rows is the caller's temporary)
    return 0;
}

void push(std::vector<int>& rows, const ethcnn_sim_thr& t) {
    for (int l = 0; l < 3; ++l) rows.push_back(t.up_k[l]);
    for (int l = 0; l < 3; ++l) rows.push_back(t.down_k[l]);
}

// checked arguments; d_out [nframes][K + 1][4]
int run_cost(ethcnn_sim* k, const ethcnn_sim_thr* ladder, int64_t K, int64_t first, int64_t per, int64_t nframes, uint32_t* d_out) {
    ethcnn_ctx* c = k->c;
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;  // the context's completion word does not cover these launches
    std::vector<int> rows;
    rows.reserve((size_t)(K + 1) * 6);
    for (int64_t i = 0; i < K; ++i) push(rows, ladder[i]);
    push(rows, sim::kFullSearch);  // column K
    if (int rc = upload_thr(k, 0, rows)) return rc;
    HIPCHK(c, hipMemsetAsync(d_out, 0, (size_t)(nframes * (K + 1)) * 16, c->stream));
    launch_cost(c->stream, k->d_recs + first * ethcnn::sim::kRecDwords, (long)per, (long)nframes, k->d_budget_thr[0], (int)(K + 1), d_out, cus_of(c));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int check_rungs(ethcnn_ctx* c, const int32_t* rung, int64_t nframes, int64_t K) {
    if (nframes && !rung) return set_err(c, ETHCNN_ERR_ARG, "null rung array");
    for (int64_t f = 0; f < nframes; ++f)
        if (rung[f] < 0 || rung[f] >= K) return set_err(c, ETHCNN_ERR_ARG, "frame %lld: rung %d outside 0..%lld", (long long)f, rung[f], (long long)(K - 1));
    return 0;
}

int upload_frame_thr(ethcnn_sim* k, const ethcnn_sim_thr* ladder, const int32_t* rung, int64_t nframes) {
    std::vector<int> rows;
    rows.reserve((size_t)nframes * 6);
    for (int64_t f = 0; f < nframes; ++f) push(rows, ladder[rung[f]]);
    return upload_thr(k, 1, rows);
}

// CTUs ctu0 .. ctu0 + n of the window whose per-frame thresholds are uploaded -> d_out (indexed from ctu0)
int run_bake(ethcnn_sim* k, int64_t first, int64_t per, int64_t ctu0, int64_t n, float* d_out) {
    ethcnn_ctx* c = k->c;
    c->done_armed = 0;
    launch_bake(c->stream, k->d_recs + first * ethcnn::sim::kRecDwords, (long)per, (long)ctu0, (long)n, k->d_budget_thr[1], d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// checked arguments -> host memory, staged in pieces through one device buffer
int bake_staged(ethcnn_sim* k, const ethcnn_sim_thr* ladder, const int32_t* rung, int64_t first, int64_t per, int64_t nframes, float* probs_out) {
    ethcnn_ctx* c = k->c;
    const int64_t n = nframes * per, row = kNout * 4;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t piece = std::min(n, k->decide_piece > 0 ? k->decide_piece : kStageCtus);
    Scratch d;
    if (int rc = d.alloc(c, (size_t)(piece * row), "search budget", true)) return rc;
    int rc = upload_frame_thr(k, ladder, rung, nframes);
    for (int64_t at = 0; at < n && !rc; at += piece) {
        const int64_t cur = std::min(piece, n - at);
        rc = run_bake(k, first, per, at, cur, d.at<float>());
        hipError_t e = hipSuccess;
        if (!rc) e = hipMemcpyAsync(probs_out + at * kNout, d.at(), (size_t)(cur * row), hipMemcpyDeviceToHost, c->stream);
        if (!rc && e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (!rc && e != hipSuccess) {
            (void)hipGetLastError();
            rc = set_err(c, ETHCNN_ERR_DEVICE, "search budget: %s", hipGetErrorString(e));
        }
    }
    return rc;
}

// checked arguments -> host memory through one device buffer
int cost_to_host(ethcnn_sim* k, const ethcnn_sim_thr* ladder, int64_t K, int64_t first, int64_t per, int64_t nframes, uint32_t* checked_out) {
    ethcnn_ctx* c = k->c;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)(nframes * (K + 1)) * 16;
    Scratch d;
    if (int rc = d.alloc(c, bytes, "search budget")) return rc;
    int rc = run_cost(k, ladder, K, first, per, nframes, d.at<uint32_t>());
    if (!rc) {
        hipError_t e = hipMemcpyAsync(checked_out, d.at(), bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            rc = set_err(c, ETHCNN_ERR_DEVICE, "search budget: %s", hipGetErrorString(e));
        }
    }
    return rc;
}
}  // namespace

extern "C" int ethcnn_budget_default_ladder(ethcnn_sim_thr* out) {
    if (!out) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_budget_default_ladder: null output");
    for (int j = 0; j < kDefaultRungs; ++j)
        for (int l = 0; l < 3; ++l) out[j].up_k[l] = 1024 - j, out[j].down_k[l] = j - 1;
    return ETHCNN_OK;
}

extern "C" int ethcnn_budget_companion_thr(ethcnn_sim_thr* out) {
    if (!out) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_budget_companion_thr: null output");
    for (int l = 0; l < 3; ++l) out->up_k[l] = 768, out->down_k[l] = 256;
    return ETHCNN_OK;
}

extern "C" int ethcnn_budget_choose(const uint32_t* checked, int64_t nframes, int64_t K, const uint64_t weight[4], uint32_t budget_ppm, int mode,
                                    int32_t* rung_out, uint8_t* over_out, uint64_t* cost_out, uint64_t* full_out) {
    if (nframes < 0 || (nframes && !checked) || !weight) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_budget_choose: null argument or negative frame count");
    if (int rc = sim::check_rung_count(nullptr, K, "ethcnn_budget_choose: ")) return rc;
    if (budget_ppm > 1000000u) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_budget_choose: the budget is in parts per million, 0..1000000: got %u", budget_ppm);
    if (mode != ETHCNN_BUDGET_FRAME && mode != ETHCNN_BUDGET_CARRY)
        return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_budget_choose: mode %d is neither ETHCNN_BUDGET_FRAME nor ETHCNN_BUDGET_CARRY", mode);
    if (int rc = sim::check_weights(nullptr, weight, "ethcnn_budget_choose: ")) return rc;
    std::vector<int32_t> rung((size_t)nframes);
    std::vector<uint8_t> over((size_t)nframes);
    std::vector<uint64_t> cost((size_t)nframes), full((size_t)nframes);
    u128 carry = 0;
    for (int64_t f = 0; f < nframes; ++f) {
        const uint32_t* row = checked + f * (K + 1) * 4;
        auto cost_of = [&](int64_t k) {
            u128 v = 0;
            for (int d = 0; d < 4; ++d) v += (u128)weight[d] * row[k * 4 + d];
            return v;
        };
        for (int64_t k = 0; k <= K; ++k)
            if (cost_of(k) >> 64)
                return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_budget_choose: the cost of frame %lld, rung %lld does not fit in 64 bits", (long long)f, (long long)k);
        const u128 allow = (u128)budget_ppm * cost_of(K) + carry;
        int64_t fit = -1, least = 0;
        for (int64_t k = 0; k < K && fit < 0; ++k) {
            if (cost_of(k) * 1000000u <= allow) fit = k;
            if (cost_of(k) < cost_of(least)) least = k;
        }
        const int64_t at = fit >= 0 ? fit : least;
        rung[(size_t)f] = (int32_t)at;
        over[(size_t)f] = fit < 0;
        cost[(size_t)f] = (uint64_t)cost_of(at);
        full[(size_t)f] = (uint64_t)cost_of(K);
        carry = mode == ETHCNN_BUDGET_CARRY && fit >= 0 ? allow - cost_of(at) * 1000000u : 0;
    }
    if (rung_out) std::copy(rung.begin(), rung.end(), rung_out);
    if (over_out) std::copy(over.begin(), over.end(), over_out);
    if (cost_out) std::copy(cost.begin(), cost.end(), cost_out);
    if (full_out) std::copy(full.begin(), full.end(), full_out);
    return ETHCNN_OK;
}

extern "C" int ethcnn_budget_cost_device(ethcnn_sim* k, const ethcnn_sim_thr* ladder, int64_t K, int64_t first, int width, int height, int64_t nframes,
                                         uint32_t* d_checked_out) {
    if (!k) return ETHCNN_ERR_ARG;
    int64_t per = 0;
    if (int rc = check_ladder(k->c, ladder, K)) return rc;
    if (int rc = check_window(k, first, width, height, nframes, &per)) return rc;
    if (nframes == 0) return ETHCNN_OK;
    if (!d_checked_out || (uintptr_t)d_checked_out % 4) return set_err(k->c, ETHCNN_ERR_ARG, "null or not 4-byte aligned device buffer");
    return run_cost(k, ladder, K, first, per, nframes, d_checked_out);
}

extern "C" int ethcnn_budget_cost(ethcnn_sim* k, const ethcnn_sim_thr* ladder, int64_t K, int64_t first, int width, int height, int64_t nframes,
                                  uint32_t* checked_out) {
    if (!k) return ETHCNN_ERR_ARG;
    int64_t per = 0;
    if (int rc = check_ladder(k->c, ladder, K)) return rc;
    if (int rc = check_window(k, first, width, height, nframes, &per)) return rc;
    if (nframes == 0) return ETHCNN_OK;
    if (!checked_out) return set_err(k->c, ETHCNN_ERR_ARG, "null output buffer");
    return cost_to_host(k, ladder, K, first, per, nframes, checked_out);
}

extern "C" int ethcnn_budget_bake_device(ethcnn_sim* k, const ethcnn_sim_thr* ladder, int64_t K, const int32_t* rung, int64_t first, int width, int height,
                                         int64_t nframes, float* d_probs_out) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    int64_t per = 0;
    if (int rc = check_ladder(c, ladder, K)) return rc;
    if (int rc = check_window(k, first, width, height, nframes, &per)) return rc;
    if (int rc = check_rungs(c, rung, nframes, K)) return rc;
    if (nframes == 0) return ETHCNN_OK;
    if (!d_probs_out || (uintptr_t)d_probs_out % 4) return set_err(c, ETHCNN_ERR_ARG, "null or not 4-byte aligned device buffer");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = upload_frame_thr(k, ladder, rung, nframes)) return rc;
    return run_bake(k, first, per, 0, nframes * per, d_probs_out);
}

extern "C" int ethcnn_budget_bake(ethcnn_sim* k, const ethcnn_sim_thr* ladder, int64_t K, const int32_t* rung, int64_t first, int width, int height,
                                  int64_t nframes, float* probs_out) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    int64_t per = 0;
    if (int rc = check_ladder(c, ladder, K)) return rc;
    if (int rc = check_window(k, first, width, height, nframes, &per)) return rc;
    if (int rc = check_rungs(c, rung, nframes, K)) return rc;
    if (nframes == 0) return ETHCNN_OK;
    if (!probs_out) return set_err(c, ETHCNN_ERR_ARG, "null output buffer");
    return bake_staged(k, ladder, rung, first, per, nframes, probs_out);
}

extern "C" int ethcnn_budget_control(ethcnn_sim* k, const ethcnn_sim_thr* ladder, int64_t K, const uint64_t weight[4], uint32_t budget_ppm, int mode,
                                     int64_t first, int width, int height, int64_t nframes, float* probs_out, int32_t* rung_out, uint8_t* over_out,
                                     uint64_t* cost_out, uint64_t* full_out) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    std::vector<ethcnn_sim_thr> dflt;
    if (!ladder) {
        dflt.resize(kDefaultRungs);
        ethcnn_budget_default_ladder(dflt.data());
        ladder = dflt.data();
        K = kDefaultRungs;
    }
    if (!weight) weight = sim::kDefaultWeight;
    int64_t per = 0;
    if (int rc = check_ladder(c, ladder, K)) return rc;
    if (int rc = check_window(k, first, width, height, nframes, &per)) return rc;
    // (the other arguments of the choice, before anything runs: an empty call checks them too)
    if (int rc = ethcnn_budget_choose(nullptr, 0, K, weight, budget_ppm, mode, nullptr, nullptr, nullptr, nullptr))
        return set_err(c, rc, "%s", ethcnn_last_error(nullptr));
    if (nframes == 0) return ETHCNN_OK;
    std::vector<uint32_t> checked((size_t)(nframes * (K + 1)) * 4);
    if (int rc = cost_to_host(k, ladder, K, first, per, nframes, checked.data())) return rc;
    std::vector<int32_t> rung((size_t)nframes);
    std::vector<uint8_t> over((size_t)nframes);
    std::vector<uint64_t> cost((size_t)nframes), full((size_t)nframes);
    if (int rc = ethcnn_budget_choose(checked.data(), nframes, K, weight, budget_ppm, mode, rung.data(), over.data(), cost.data(), full.data()))
        return set_err(c, rc, "%s", ethcnn_last_error(nullptr));
    if (probs_out)
        if (int rc = bake_staged(k, ladder, rung.data(), first, per, nframes, probs_out)) return rc;
    if (rung_out) std::copy(rung.begin(), rung.end(), rung_out);
    if (over_out) std::copy(over.begin(), over.end(), over_out);
    if (cost_out) std::copy(cost.begin(), cost.end(), cost_out);
    if (full_out) std::copy(full.begin(), full.end(), full_out);
    return ETHCNN_OK;
}
