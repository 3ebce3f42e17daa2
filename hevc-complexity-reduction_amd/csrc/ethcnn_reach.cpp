// ethcnn_reach.cpp -- host side of the threshold calibration on reached nodes (include/ethcnn.h "threshold calibration on reached
// nodes"): the histogram entry around k_reach_hist (ethcnn_reach.hip) and the top-down choice, which is three such histograms and
// ethcnn_calib_choose on each.
#include "ethcnn_analysis.h"
#include "ethcnn_reach.h"

using ethcnn::reach::kHistWords;
using ethcnn::reach::kMaxCand;

extern "C" int ethcnn_reach_hist(ethcnn_sim* k, const ethcnn_sim_thr* cand, int64_t ncand, int gate_order, uint64_t* hist) {
    static_assert(kHistWords == ETHCNN_REACH_HIST_WORDS && kMaxCand == ETHCNN_REACH_MAX_CAND && sizeof(ethcnn_sim_thr) == 24, "the kernel writes these layouts");
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (ncand < 0 || ncand > kMaxCand) return set_err(c, ETHCNN_ERR_ARG, "candidate count %lld outside 0..%d", (long long)ncand, kMaxCand);
    if (ncand == 0) return ETHCNN_OK;
    if (!cand || !hist) return set_err(c, ETHCNN_ERR_ARG, "null buffer");
    if (int rc = ethcnn::sim::check_gates(c, gate_order)) return rc;
    for (int64_t i = 0; i < ncand; ++i)
        if (int rc = ethcnn::sim::check_cand(c, cand[i], (long long)i)) return rc;
    const size_t cand_bytes = (size_t)ncand * 24, out_bytes = (size_t)ncand * kHistWords * 8;
    std::memset(hist, 0, out_bytes);
    if (k->labelled == 0) return ETHCNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;  // the context's completion word does not cover this launch
    Scratch d;  // candidates, then their histograms: one allocation, both 8-byte aligned
    if (int rc = d.alloc(c, cand_bytes + out_bytes, "reached nodes")) return rc;
    hipError_t e = hipMemcpyAsync(d.at(), cand, cand_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d.at(cand_bytes), 0, out_bytes, c->stream);
    if (e == hipSuccess) {
        ethcnn::reach::launch_hist(c->stream, k->d_recs, k->d_m, (long)k->ctus, d.at<const int>(), (long)ncand, gate_order,
                                   d.at<unsigned long long>(cand_bytes), cus_of(c));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hist, d.at(cand_bytes), out_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, ETHCNN_ERR_DEVICE, "reached nodes: %s", hipGetErrorString(e));
    }
    return ETHCNN_OK;
}

extern "C" int ethcnn_reach_calibrate(ethcnn_sim* k, const uint32_t eps_down_ppm[3], const uint32_t eps_up_ppm[3], int gate_order, ethcnn_calib_report* report,
                                      ethcnn_sim_thr* thr_out, ethcnn_sim_counts* counts_out) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (!eps_down_ppm || !eps_up_ppm || !report || !thr_out) return set_err(c, ETHCNN_ERR_ARG, "null argument");
    for (int l = 0; l < 3; ++l)
        if (eps_down_ppm[l] > 1000000u || eps_up_ppm[l] > 1000000u)
            return set_err(c, ETHCNN_ERR_ARG, "a budget is in parts per million, 0..1000000 (level %d: %u / %u)", l + 1, eps_down_ppm[l], eps_up_ppm[l]);
    if (int rc = ethcnn::sim::check_gates(c, gate_order)) return rc;
    if (k->labelled == 0) return set_err(c, ETHCNN_ERR_ARG, "the calibration needs labelled CTUs: the set holds none");
    ethcnn_sim_thr thr = ethcnn::sim::kFullSearch;
    ethcnn_calib_report rep, at;
    std::vector<uint64_t> hist((size_t)kHistWords);
    for (int l = 0; l < 3; ++l) {  // top-down: level l is chosen on the nodes reached under the levels above it
        if (int rc = ethcnn_reach_hist(k, &thr, 1, gate_order, hist.data())) return rc;
        if (int rc = ethcnn_calib_choose(hist.data(), eps_down_ppm, eps_up_ppm, &at)) return set_err(c, rc, "%s", ethcnn_last_error(nullptr));
        rep.level[l] = at.level[l];
        thr.up_k[l] = at.level[l].up_k;
        thr.down_k[l] = at.level[l].down_k;
    }
    ethcnn_sim_counts counts;
    if (counts_out)
        if (int rc = ethcnn_sim_eval(k, &thr, 1, gate_order, &counts)) return rc;
    *report = rep;
    *thr_out = thr;
    if (counts_out) *counts_out = counts;
    return ETHCNN_OK;
}
