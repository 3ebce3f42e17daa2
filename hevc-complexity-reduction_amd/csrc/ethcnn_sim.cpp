// ethcnn_sim.cpp -- host side of the partition-search simulator (include/ethcnn.h "partition-search simulation"): the set object, its
// add / eval entries around the kernels of ethcnn_sim.hip, and the sweep and the coordinate-descent search built from evaluations.
#include "ethcnn_analysis.h"
#include "ethcnn_calib.h"

using namespace ethcnn::sim;

namespace {
constexpr int64_t kMaxCand = 1 << 26;

// room for `ctus` more records and `subs` more sub-batches; the set's content moves to the new buffers, nothing else changes
int reserve(ethcnn_sim* k, int64_t ctus, int64_t subs) {
    ethcnn_ctx* c = k->c;
    if (k->subs + subs > (int64_t)1 << 31) return set_err(c, ETHCNN_ERR_ARG, "simulation: more than 2^31 sub-batches");
    if (k->ctus + ctus > k->cap_ctus) {
        const int64_t cap = std::max(k->ctus + ctus, k->cap_ctus * 2);
        unsigned* p = nullptr;
        if (hipMalloc((void**)&p, (size_t)cap * kRecDwords * 4) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(c, ETHCNN_ERR_NOMEM, "simulation: %lld bytes for %lld CTU records do not fit in device memory", (long long)(cap * kRecDwords * 4),
                           (long long)cap);
        }
        hipError_t e = k->ctus ? hipMemcpyAsync(p, k->d_recs, (size_t)k->ctus * kRecDwords * 4, hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return set_err(c, ETHCNN_ERR_DEVICE, "simulation: %s", hipGetErrorString(e));
        }
        if (k->d_recs) (void)hipFree(k->d_recs);
        k->d_recs = p;
        k->cap_ctus = cap;
    }
    if (k->subs + subs > k->cap_subs) {
        const int64_t cap = std::max(k->subs + subs, k->cap_subs * 2);
        unsigned* p = nullptr;
        if (hipMalloc((void**)&p, (size_t)cap * 8) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(c, ETHCNN_ERR_NOMEM, "simulation: %lld bytes for %lld sub-batches do not fit in device memory", (long long)(cap * 8), (long long)cap);
        }
        const unsigned none[2] = {kNoGate, kNoGate};
        hipError_t e = k->d_m ? hipMemcpyAsync(p, k->d_m, (size_t)k->subs * 8, hipMemcpyDeviceToDevice, c->stream)
                              : hipMemcpyAsync(p, none, 8, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return set_err(c, ETHCNN_ERR_DEVICE, "simulation: %s", hipGetErrorString(e));
        }
        if (k->d_m) (void)hipFree(k->d_m);
        k->d_m = p;
        k->cap_subs = cap;
    }
    return 0;
}

// An add in flight: `units` CTUs (per-CTU layout) or frames go behind the set piece by piece; commit() makes them part of it.
struct Add {
    ethcnn_sim* k;
    Geom g;
    int64_t per, subs_per_unit;  // CTUs / sub-batches a unit
    int64_t done = 0;            // units packed so far
    uint64_t whole = 0, labelled = 0, rejected = 0, bad = 0;

    int begin(int64_t units) {
        ethcnn_ctx* c = k->c;
        HIPCHK(c, hipSetDevice(c->device));
        c->done_armed = 0;  // the context's completion word does not cover these launches
        if (int rc = reserve(k, units * per, units * subs_per_unit)) return rc;
        if (subs_per_unit) HIPCHK(c, hipMemsetAsync(k->d_m + 2 * k->subs, 0, (size_t)(units * subs_per_unit) * 8, c->stream));
        return 0;
    }
    // m units that are in HBM
    int pack(const float* d_probs, const uint8_t* d_labels, int64_t m) {
        ethcnn_ctx* c = k->c;
        hipError_t e = hipMemsetAsync(k->d_call, 0, kCallWords * 8, c->stream);
        if (e == hipSuccess) {
            launch_pack(c->stream, d_probs, d_labels, (long)(m * per), g, (unsigned)(k->subs + done * subs_per_unit),
                        k->d_recs + (k->ctus + done * per) * kRecDwords, k->d_m, k->d_call, cus_of(c));
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(k->h_call, k->d_call, kCallWords * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return set_err(c, ETHCNN_ERR_DEVICE, "simulation: %s", hipGetErrorString(e));
        }
        bad += k->h_call[kCallFlag];
        whole += k->h_call[kCallWhole];
        labelled += k->h_call[kCallLabelled];
        rejected += k->h_call[kCallRejected];
        done += m;
        return 0;
    }
    int commit() {
        if (bad) return set_err(k->c, ETHCNN_ERR_FORMAT, "%llu CTU(s) hold a depth byte above 3 (CU depths are 0..3); nothing was added", (unsigned long long)bad);
        if (g.ctus_w && done) {  // a run of whole frames: joined to the run in front of it when that has the same geometry
            if (!k->runs.empty() && k->runs.back().width == g.width && k->runs.back().height == g.height &&
                k->runs.back().first + k->runs.back().nframes * per == k->ctus)
                k->runs.back().nframes += done;
            else
                k->runs.push_back({k->ctus, g.width, g.height, done});
        }
        k->ctus += done * per;
        k->subs += done * subs_per_unit;
        k->whole += whole;
        k->labelled += labelled;
        k->rejected += rejected;
        return ETHCNN_OK;
    }
};

// host pointers: pieces of `piece` units go through a device buffer; pb / lb = bytes of probabilities / labels per unit
int add_staged(Add& a, const float* probs, const uint8_t* labels, int64_t units, int64_t piece, int64_t pb, int64_t lb) {
    if (int rc = a.begin(units)) return rc;
    Scratch stage;
    if (int rc = stage_pieces(a.k->c, stage, "simulation", probs, labels, units, piece, pb, lb,
                              [&](const float* d_p, const uint8_t* d_l, int64_t m) { return a.pack(d_p, d_l, m); }))
        return rc;
    return a.commit();
}

int sim_geom(ethcnn_ctx* c, int width, int height, bool labels, Geom* g) {
    PicSize s;
    if (int rc = check_size(c, width, height, labels ? 16 : 8, &s)) return rc;
    *g = Geom{s.ctus_w, s.ctus_h, width, height, s.w16, s.h16, (s.ctus_w * s.ctus_h + 1023) / 1024};
    return 0;
}

int& coord_of(ethcnn_sim_thr& t, int coord) { return coord & 1 ? t.up_k[coord >> 1] : t.down_k[coord >> 1]; }

u128 cost_of(const ethcnn_sim_counts& n, const uint64_t weight[4]) {
    u128 v = 0;
    for (int d = 0; d < 4; ++d) v += (u128)weight[d] * n.checked[d];
    return v;
}
}  // namespace

extern "C" int ethcnn_sim_create(ethcnn_ctx* c, ethcnn_sim** out) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "null output pointer");
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    ethcnn_sim* k = new (std::nothrow) ethcnn_sim;
    if (!k) return set_err(c, ETHCNN_ERR_NOMEM, "out of memory");
    k->c = c;
    hipError_t e = hipMalloc((void**)&k->d_call, kCallWords * 8);
    if (e == hipSuccess) e = hipHostMalloc((void**)&k->h_call, kCallWords * 8, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ethcnn_sim_destroy(k);
        return set_err(c, ETHCNN_ERR_DEVICE, "simulator: %s", hipGetErrorString(e));
    }
    if (int rc = reserve(k, 0, 0)) {  // the "no sub-batch" entry
        ethcnn_sim_destroy(k);
        return rc;
    }
    *out = k;
    return ETHCNN_OK;
}

extern "C" void ethcnn_sim_destroy(ethcnn_sim* k) {
    if (!k) return;
    (void)hipSetDevice(k->c->device);
    (void)hipStreamSynchronize(k->c->stream);
    if (k->d_recs) (void)hipFree(k->d_recs);
    if (k->d_m) (void)hipFree(k->d_m);
    if (k->d_call) (void)hipFree(k->d_call);
    if (k->d_cand) (void)hipFree(k->d_cand);
    if (k->d_out) (void)hipFree(k->d_out);
    for (int* p : k->d_budget_thr)
        if (p) (void)hipFree(p);
    if (k->d_rel) (void)hipFree(k->d_rel);
    if (k->h_call) (void)hipHostFree(k->h_call);
    delete k;
}

extern "C" int ethcnn_sim_reset(ethcnn_sim* k) {
    if (!k) return ETHCNN_ERR_ARG;
    k->ctus = 0;
    k->subs = 1;
    k->whole = k->labelled = k->rejected = 0;
    k->runs.clear();
    return ETHCNN_OK;
}

extern "C" int ethcnn_sim_add_device(ethcnn_sim* k, const float* d_probs, const uint8_t* d_depth16, int64_t n) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (n < 0) return set_err(c, ETHCNN_ERR_ARG, "negative CTU count %lld", (long long)n);
    if (n == 0) return ETHCNN_OK;
    if (!d_probs || ((uintptr_t)d_probs | (uintptr_t)d_depth16) % 4) return set_err(c, ETHCNN_ERR_ARG, "null or not 4-byte aligned device buffer");
    Add a{k, {0, 0, 64, 64, 0, 0, 0}, 1, 0};
    if (int rc = a.begin(n)) return rc;
    if (int rc = a.pack(d_probs, d_depth16, n)) return rc;
    return a.commit();
}

extern "C" int ethcnn_sim_add(ethcnn_sim* k, const float* probs, const uint8_t* depth16, int64_t n) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (n < 0) return set_err(c, ETHCNN_ERR_ARG, "negative CTU count %lld", (long long)n);
    if (n == 0) return ETHCNN_OK;
    if (!probs) return set_err(c, ETHCNN_ERR_ARG, "null buffer");
    Add a{k, {0, 0, 64, 64, 0, 0, 0}, 1, 0};
    return add_staged(a, probs, depth16, n, kStageCtus, 84, 16);
}

extern "C" int ethcnn_sim_add_frames_device(ethcnn_sim* k, const float* d_probs, const uint8_t* d_labels, int width, int height, int64_t nframes,
                                            int64_t skip_label_frames) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    Geom g;
    if (int rc = sim_geom(c, width, height, d_labels != nullptr, &g)) return rc;
    if (nframes < 0 || skip_label_frames < 0) return set_err(c, ETHCNN_ERR_ARG, "negative frame count");
    if (nframes == 0) return ETHCNN_OK;
    if (!d_probs || (uintptr_t)d_probs % 4) return set_err(c, ETHCNN_ERR_ARG, "null or misaligned device buffer");
    Add a{k, g, (int64_t)g.ctus_w * g.ctus_h, g.subs};
    if (int rc = a.begin(nframes)) return rc;
    if (int rc = a.pack(d_probs, d_labels ? d_labels + skip_label_frames * g.w16 * g.h16 : nullptr, nframes)) return rc;
    return a.commit();
}

extern "C" int ethcnn_sim_add_frames(ethcnn_sim* k, const float* probs, const uint8_t* labels, int width, int height, int64_t nframes,
                                     int64_t skip_label_frames) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    Geom g;
    if (int rc = sim_geom(c, width, height, labels != nullptr, &g)) return rc;
    if (nframes < 0 || skip_label_frames < 0) return set_err(c, ETHCNN_ERR_ARG, "negative frame count");
    if (nframes == 0) return ETHCNN_OK;
    if (!probs) return set_err(c, ETHCNN_ERR_ARG, "null buffer");
    const int64_t per = (int64_t)g.ctus_w * g.ctus_h, lab = (int64_t)g.w16 * g.h16;
    Add a{k, g, per, g.subs};
    return add_staged(a, probs, labels ? labels + skip_label_frames * lab : nullptr, nframes, std::max<int64_t>(1, kStageCtus / per), per * 84, lab);
}

extern "C" int ethcnn_sim_info(ethcnn_sim* k, ethcnn_sim_set_info* info) {
    if (!k) return ETHCNN_ERR_ARG;
    if (!info) return set_err(k->c, ETHCNN_ERR_ARG, "null output pointer");
    info->ctus = (uint64_t)k->ctus;
    info->whole_ctus = k->whole;
    info->labelled_ctus = k->labelled;
    info->rejected_ctus = k->rejected;
    info->sub_batches = (uint64_t)(k->subs - 1);
    return ETHCNN_OK;
}

extern "C" int ethcnn_sim_eval(ethcnn_sim* k, const ethcnn_sim_thr* cand, int64_t ncand, int gate_order, ethcnn_sim_counts* out) {
    static_assert(sizeof(ethcnn_sim_counts) == kFields * 8 && sizeof(ethcnn_sim_thr) == 24, "the kernel writes these layouts");
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (ncand < 0 || ncand > kMaxCand) return set_err(c, ETHCNN_ERR_ARG, "candidate count %lld outside 0..%lld", (long long)ncand, (long long)kMaxCand);
    if (ncand == 0) return ETHCNN_OK;
    if (!cand || !out) return set_err(c, ETHCNN_ERR_ARG, "null buffer");
    if (int rc = check_gates(c, gate_order)) return rc;
    for (int64_t i = 0; i < ncand; ++i)
        if (int rc = check_cand(c, cand[i], (long long)i)) return rc;
    std::memset(out, 0, (size_t)ncand * sizeof *out);
    if (k->ctus == 0) return ETHCNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;
    if (ncand > k->cap_cand) {
        int* d_cand = nullptr;
        unsigned long long* d_out = nullptr;
        if (hipMalloc((void**)&d_cand, (size_t)ncand * 24) != hipSuccess || hipMalloc((void**)&d_out, (size_t)ncand * kFields * 8) != hipSuccess) {
            (void)hipGetLastError();
            if (d_cand) (void)hipFree(d_cand);
            return set_err(c, ETHCNN_ERR_NOMEM, "simulation: %lld bytes for %lld candidates do not fit in device memory", (long long)(ncand * (24 + kFields * 8)),
                           (long long)ncand);
        }
        if (k->d_cand) (void)hipFree(k->d_cand);
        if (k->d_out) (void)hipFree(k->d_out);
        k->d_cand = d_cand;
        k->d_out = d_out;
        k->cap_cand = ncand;
    }
    HIPCHK(c, hipMemcpyAsync(k->d_cand, cand, (size_t)ncand * 24, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(k->d_out, 0, (size_t)ncand * kFields * 8, c->stream));
    launch_eval(c->stream, k->d_recs, k->d_m, (long)k->ctus, k->d_cand, (long)ncand, gate_order, k->d_out, cus_of(c));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, k->d_out, (size_t)ncand * kFields * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ETHCNN_OK;
}

extern "C" int ethcnn_sim_sweep(ethcnn_sim* k, const ethcnn_sim_thr* base, int coord, int gate_order, ethcnn_sim_counts* out) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (!base || !out) return set_err(c, ETHCNN_ERR_ARG, "null buffer");
    if (coord < 0 || coord > 5) return set_err(c, ETHCNN_ERR_ARG, "coordinate %d outside 0..5 (down0, up0, down1, up1, down2, up2)", coord);
    const int lo = coord & 1 ? 0 : -1, count = 1025 - lo;
    std::vector<ethcnn_sim_thr> cand((size_t)count, *base);
    for (int i = 0; i < count; ++i) coord_of(cand[(size_t)i], coord) = lo + i;
    return ethcnn_sim_eval(k, cand.data(), count, gate_order, out);
}

extern "C" int ethcnn_sim_search(ethcnn_sim* k, const ethcnn_sim_thr* start, int gate_order, const uint64_t weight[4], uint32_t max_bad_ppm, int max_rounds,
                                 ethcnn_sim_thr* thr_out, ethcnn_sim_counts* counts_out, int* rounds_out) {
    if (!k) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = k->c;
    if (!start || !weight || !thr_out) return set_err(c, ETHCNN_ERR_ARG, "null argument");
    if (max_bad_ppm > 1000000u) return set_err(c, ETHCNN_ERR_ARG, "the share of bad CTUs is in parts per million, 0..1000000: got %u", max_bad_ppm);
    if (max_rounds < 0) return set_err(c, ETHCNN_ERR_ARG, "negative number of rounds %d", max_rounds);
    if (k->labelled == 0) return set_err(c, ETHCNN_ERR_ARG, "the search needs labelled CTUs: the set holds none");
    const u128 budget = (u128)max_bad_ppm * k->labelled;
    auto feasible = [&](const ethcnn_sim_counts& n) { return (u128)n.bad_ctus * 1000000u <= budget; };
    ethcnn_sim_thr cur = *start;
    ethcnn_sim_counts at;
    if (int rc = ethcnn_sim_eval(k, &cur, 1, gate_order, &at)) return rc;
    if (!feasible(at))
        return set_err(c, ETHCNN_ERR_ARG, "the search starts from a feasible point: %llu bad of %llu labelled CTUs is above %u ppm", (unsigned long long)at.bad_ctus,
                       (unsigned long long)k->labelled, max_bad_ppm);
    std::vector<ethcnn_sim_counts> line(ETHCNN_SIM_SWEEP_MAX);
    int rounds = 0;
    for (bool changed = true; changed && rounds < max_rounds; ++rounds) {
        changed = false;
        for (int coord = 0; coord < 6; ++coord) {
            if (int rc = ethcnn_sim_sweep(k, &cur, coord, gate_order, line.data())) return rc;
            const int lo = coord & 1 ? 0 : -1, count = 1025 - lo;
            int best = -1;  // (the current value is feasible, so one is found)
            for (int i = 0; i < count; ++i)
                if (feasible(line[(size_t)i]) && (best < 0 || cost_of(line[(size_t)i], weight) < cost_of(line[(size_t)best], weight))) best = i;
            if (lo + best != coord_of(cur, coord)) {
                coord_of(cur, coord) = lo + best;
                changed = true;
            }
            at = line[(size_t)best];
        }
    }
    *thr_out = cur;
    if (counts_out) *counts_out = at;
    if (rounds_out) *rounds_out = rounds;
    return ETHCNN_OK;
}

extern "C" int ethcnn_sim_write_thr_info(const char* path, const ethcnn_sim_thr* thr, int order) {
    if (!path || !thr) return set_err(nullptr, ETHCNN_ERR_ARG, "ethcnn_sim_write_thr_info: null argument");
    return ethcnn::calib::write_thr_line(path, thr->down_k, thr->up_k, order, "ethcnn_sim_write_thr_info");
}
