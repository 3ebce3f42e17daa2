// ethcnn_replay.cpp -- host side of the sample-set replay (include/ethcnn.h "sample-set replay"): the plan (runs, their validation, the
// source table), the replay object (open, memory plan, the chunk loop uncut -> ethcnn_ldp_sequence_device) and the two hand-offs to the
// calibrator and the partition-search simulator.  Kernels: ethcnn_replay.hip.
#include "ethcnn_analysis.h"
#include "ethcnn_calib.h"
#include "ethcnn_ldp_set.h"
#include "ethcnn_replay.h"
#include "ethcnn_samples.h"

#include <unordered_map>

using namespace ethcnn::replay;

namespace ethcnn {
namespace replay {

namespace {
std::string fmt(const char* f, ...) {
    char buf[640];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}
struct Entry {
    int run;       // position in the final run order
    uint64_t key;  // (f * nctu + line * C + col): the place in the run's [f][line][col] order
    int64_t idx;
};
std::string run_name(const Run& r) { return fmt("run (seq %d, %dx%d)", r.seq, r.w, r.h); }
}  // namespace

// Rules are checked in the order of include/ethcnn.h over the WHOLE input; the first rule that is broken anywhere is reported with the
// lowest record index that shows it.
bool plan(const Header* h, int64_t n, Plan* out, std::string* why) {
    out->runs.clear();
    out->src.clear();
    if (n <= 0) {
        *why = "no records";
        return false;
    }
    // rules "geometry" and "outside": per record
    int64_t bad_geom = -1, bad_pos = -1;
    for (int64_t i = 0; i < n && bad_geom < 0; ++i) {
        const int w = (int)(h[i].wh & 0xffff), ht = (int)(h[i].wh >> 16);
        if (w < 64 || ht < 64 || h[i].f > 0x7fffffffu) bad_geom = i;
        else if (bad_pos < 0 && ((int)(h[i].linecol & 0xffff) >= ht / 64 || (int)(h[i].linecol >> 16) >= w / 64)) bad_pos = i;
    }
    if (bad_geom >= 0) {
        const Header& b = h[bad_geom];
        *why = fmt("record %lld breaks rule 'geometry': a %ux%u picture at frame %u (width and height hold at least one whole CTU, frame numbers stay below 2^31)",
                   (long long)bad_geom, b.wh & 0xffff, b.wh >> 16, b.f);
        return false;
    }
    if (bad_pos >= 0) {
        const Header& b = h[bad_pos];
        *why = fmt("record %lld breaks rule 'outside': CTU (line %u, col %u) is not among the %u x %u whole CTUs of a %ux%u picture", (long long)bad_pos,
                   b.linecol & 0xffff, b.linecol >> 16, (b.wh >> 16) / 64, (b.wh & 0xffff) / 64, b.wh & 0xffff, b.wh >> 16);
        return false;
    }
    // runs: maximal sets of records with the same (seq, w, h), by seq, then by first appearance
    std::unordered_map<uint64_t, int> seen;
    std::vector<int64_t> first;  // first record of run k (order of appearance)
    std::vector<int> run_of((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t key = (uint64_t)h[i].seq << 32 | h[i].wh;
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (int)first.size()).first;
            first.push_back(i);
        }
        run_of[(size_t)i] = it->second;
    }
    const int nruns = (int)first.size();
    std::vector<int> order((size_t)nruns), pos((size_t)nruns);
    for (int k = 0; k < nruns; ++k) order[(size_t)k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return h[first[(size_t)a]].seq < h[first[(size_t)b]].seq; });
    std::vector<Run> runs((size_t)nruns);
    for (int p = 0; p < nruns; ++p) {
        const int k = order[(size_t)p];
        pos[(size_t)k] = p;
        const Header& a = h[first[(size_t)k]];
        Run& r = runs[(size_t)p];
        r.seq = (int)a.seq;
        r.w = (int)(a.wh & 0xffff);
        r.h = (int)(a.wh >> 16);
        r.C = r.w / 64;
        r.R = r.h / 64;
        r.nctu = (int64_t)r.R * r.C;
        for (int s = 0; s < 4; ++s) r.qp[s] = (int)(a.qps >> (8 * s) & 255);
    }
    // rule "QP differs": every record carries the slot QPs of its run's first record
    for (int64_t i = 0; i < n; ++i) {
        const int64_t f0 = first[(size_t)run_of[(size_t)i]];
        if (h[i].qps != h[f0].qps) {
            *why = fmt("record %lld breaks rule 'QP differs': slot QPs %u %u %u %u, but %u %u %u %u in record %lld, the first of its %s", (long long)i,
                       h[i].qps & 255, h[i].qps >> 8 & 255, h[i].qps >> 16 & 255, h[i].qps >> 24, h[f0].qps & 255, h[f0].qps >> 8 & 255,
                       h[f0].qps >> 16 & 255, h[f0].qps >> 24, (long long)f0, run_name(runs[(size_t)pos[(size_t)run_of[(size_t)i]]]).c_str());
            return false;
        }
    }
    // rule "QPs not distinct": shown by the run's first record (runs in order of appearance = ascending first record)
    for (int k = 0; k < nruns; ++k) {
        const Run& r = runs[(size_t)pos[(size_t)k]];
        bool same = false;
        for (int a = 0; a < 4; ++a)
            for (int b = a + 1; b < 4; ++b) same = same || r.qp[a] == r.qp[b];
        if (same) {
            *why = fmt("record %lld breaks rule 'QPs not distinct': the four slot QPs of %s are %d %d %d %d", (long long)first[(size_t)k], run_name(r).c_str(),
                       r.qp[0], r.qp[1], r.qp[2], r.qp[3]);
            return false;
        }
    }
    // every record at its place in its run
    std::vector<Entry> e((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int p = pos[(size_t)run_of[(size_t)i]];
        const Run& r = runs[(size_t)p];
        e[(size_t)i] = {p, (uint64_t)h[i].f * (uint64_t)r.nctu + (uint64_t)(h[i].linecol & 0xffff) * (uint64_t)r.C + (h[i].linecol >> 16), i};
    }
    std::sort(e.begin(), e.end(), [](const Entry& a, const Entry& b) { return a.run != b.run ? a.run < b.run : a.key != b.key ? a.key < b.key : a.idx < b.idx; });
    // rule "duplicate": shown by the later record of a pair
    int64_t dup = -1, dup_first = -1;
    for (int64_t k = 1; k < n; ++k)
        if (e[(size_t)k].run == e[(size_t)k - 1].run && e[(size_t)k].key == e[(size_t)k - 1].key && (dup < 0 || e[(size_t)k].idx < dup)) {
            dup = e[(size_t)k].idx;
            int64_t j = k - 1;  // the first of the equal keys
            while (j > 0 && e[(size_t)j - 1].run == e[(size_t)k].run && e[(size_t)j - 1].key == e[(size_t)k].key) --j;
            dup_first = e[(size_t)j].idx;
        }
    if (dup >= 0) {
        const Header& b = h[dup];
        *why = fmt("record %lld breaks rule 'duplicate': (frame %u, line %u, col %u) of %s is already held by record %lld", (long long)dup, b.f,
                   b.linecol & 0xffff, b.linecol >> 16, run_name(runs[(size_t)pos[(size_t)run_of[(size_t)dup]]]).c_str(), (long long)dup_first);
        return false;
    }
    // rule "missing": the frame numbers of a run form one range f0..f1 and every (f, line, col) of it occurs.  Shown by the run's
    // lowest record whose frame number is not below the first missing place's.
    int64_t miss = -1;
    std::string miss_why;
    for (int64_t k = 0; k < n;) {
        const int p = e[(size_t)k].run;
        Run& r = runs[(size_t)p];
        int64_t end = k;
        while (end < n && e[(size_t)end].run == p) ++end;
        const uint64_t base = (uint64_t)h[e[(size_t)k].idx].f * (uint64_t)r.nctu;  // the run's first frame starts here
        const uint32_t f1 = h[e[(size_t)end - 1].idx].f;
        int64_t j = k;
        while (j < end && e[(size_t)j].key == base + (uint64_t)(j - k)) ++j;
        if (j < end || (uint64_t)(end - k) % (uint64_t)r.nctu) {
            const uint64_t want = base + (uint64_t)(j - k);
            const uint32_t f = (uint32_t)(want / (uint64_t)r.nctu);
            const int ctu = (int)(want % (uint64_t)r.nctu);
            int64_t shown = -1;
            for (int64_t q = k; q < end; ++q)
                if (h[e[(size_t)q].idx].f >= f && (shown < 0 || e[(size_t)q].idx < shown)) shown = e[(size_t)q].idx;
            if (miss < 0 || shown < miss) {
                miss = shown;
                miss_why = fmt("record %lld breaks rule 'missing': %s lacks (frame %u, line %d, col %d) of its frame range %u..%u", (long long)shown,
                               run_name(r).c_str(), f, ctu / r.C, ctu % r.C, h[e[(size_t)k].idx].f, f1);
            }
        }
        r.f0 = h[e[(size_t)k].idx].f;
        r.F = (end - k) / r.nctu;
        r.src_at = k;
        k = end;
    }
    if (miss >= 0) {
        *why = miss_why;
        return false;
    }
    out->src.resize((size_t)n);
    for (int64_t k = 0; k < n; ++k) out->src[(size_t)k] = e[(size_t)k].idx;
    out->runs = std::move(runs);
    return true;
}

}  // namespace replay
}  // namespace ethcnn

namespace {
constexpr size_t kIoBytes = 64u << 20;              // upload piece of host records
constexpr int64_t kChunkBytes = (int64_t)256 << 20;  // default chunk: this much of residual planes

int rerr(ethcnn_replay* p, int code, const char* fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    p->err = buf;
    return code;
}

void fill_run(const Run& r, ethcnn_replay_run* o) {
    o->seq = r.seq;
    o->w = r.w;
    o->h = r.h;
    o->rows = r.R;
    o->cols = r.C;
    o->f0 = r.f0;
    o->frames = r.F;
    o->nctu = r.nctu;
    for (int s = 0; s < 4; ++s) o->qp[s] = r.qp[s];
    o->src_offset = r.src_at;
}

template <typename T>
void free_buf(T*& p, size_t& cap) {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}

// everything the object holds in HBM goes (the stream is drained first)
void close_all(ethcnn_replay* p) {
    if (p->own || p->d_resi || p->d_src || p->d_probs || p->d_labels || p->d_zero) (void)hipStreamSynchronize(p->c->stream);
    size_t none = 0;
    free_buf(p->own, none);
    free_buf(p->d_resi, p->resi_cap);
    free_buf(p->d_src, p->src_cap);
    free_buf(p->d_probs, p->probs_cap);
    free_buf(p->d_labels, p->labels_cap);
    free_buf(p->d_zero, p->zero_cap);
    p->rec = nullptr;
    p->nrec = 0;
    p->plan.runs.clear();
    p->plan.src.clear();
    p->src_run = -1;
}

int64_t chunk_frames(const ethcnn_replay* p, const Run& r) {
    const int64_t def = std::max<int64_t>(1, kChunkBytes / (r.nctu * 4096));
    return std::min<int64_t>(r.F, p->chunk > 0 ? (int64_t)p->chunk : def);
}

struct Need {
    size_t rec, resi, src, probs, labels, zero;
    unsigned long long total() const { return (unsigned long long)rec + resi + src + probs + labels + zero; }
};
Need need_of(const ethcnn_replay* p, const Run& r, bool own_probs, bool own_labels, int nslots = 1) {
    Need n;
    n.rec = p->own ? (size_t)p->nrec * kRec : 0;
    n.resi = (size_t)nslots * (size_t)(chunk_frames(p, r) * r.nctu) * 4096;  // the chunk's planes of every slot replayed together
    n.src = (size_t)(r.F * r.nctu) * 8;
    n.probs = own_probs ? (size_t)(r.F * r.nctu) * kNOut * 4 : 0;
    n.labels = own_labels ? (size_t)(r.F * r.nctu) * 16 : 0;
    n.zero = r.f0 > 1 ? (size_t)r.nctu * 2 * kNVec * 4 : 0;
    return n;
}

int check_run(ethcnn_replay* p, int run, int slot) {
    if (p->plan.runs.empty()) return rerr(p, ETHCNN_ERR_ARG, "nothing is open (ethcnn_replay_open_set / ethcnn_replay_open_records)");
    if (run < 0 || run >= (int)p->plan.runs.size()) return rerr(p, ETHCNN_ERR_ARG, "run %d outside 0..%d", run, (int)p->plan.runs.size() - 1);
    if (slot < 0 || slot > 3) return rerr(p, ETHCNN_ERR_ARG, "QP slot %d outside 0..3", slot);
    return 0;
}

// the object's buffers at exactly the sizes of `nd` (what is held is what was checked); refuses with the whole sum before it allocates
// what it cannot get.  what: "run 3 (5 frames of 12 CTUs)", for the messages
int ensure_buffers(ethcnn_replay* p, const Need& nd, const char* what) {
    ethcnn_ctx* c = p->c;
    const unsigned long long total = nd.total();
    if (p->max_bytes && total > p->max_bytes)
        return rerr(p, ETHCNN_ERR_NOMEM, "%s needs %llu bytes on the device, above the object's limit of %llu", what, total, (unsigned long long)p->max_bytes);
    // buffers of exactly this run's sizes: what is held is what was checked
    const size_t want[5] = {nd.resi, nd.src, nd.probs, nd.labels, nd.zero};
    size_t* cap[5] = {&p->resi_cap, &p->src_cap, &p->probs_cap, &p->labels_cap, &p->zero_cap};
    void** buf[5] = {(void**)&p->d_resi, (void**)&p->d_src, (void**)&p->d_probs, (void**)&p->d_labels, (void**)&p->d_zero};
    size_t grow = 0, back = 0;
    for (int k = 0; k < 5; ++k)
        if (*cap[k] != want[k]) grow += want[k], back += *cap[k];
    if (grow || back) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "hipMemGetInfo failed");
        if (grow > free_b + back)
            return rerr(p, ETHCNN_ERR_NOMEM, "%s needs %llu bytes on the device; %zu are free", what, total, free_b + back);
        if (hipStreamSynchronize(c->stream) != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "hipStreamSynchronize failed");
        for (int k = 0; k < 5; ++k)
            if (*cap[k] != want[k]) {
                if (*buf[k]) (void)hipFree(*buf[k]);
                *buf[k] = nullptr;
                *cap[k] = 0;
                if (k == 1) p->src_run = -1;
            }
        for (int k = 0; k < 5; ++k)
            if (want[k] && !*buf[k]) {
                if (hipMalloc(buf[k], want[k]) != hipSuccess) {
                    (void)hipGetLastError();
                    *buf[k] = nullptr;
                    return rerr(p, ETHCNN_ERR_NOMEM, "%s needs %llu bytes on the device: %zu of them do not fit", what, total, want[k]);
                }
                *cap[k] = want[k];
                if (k == 4 && hipMemsetAsync(*buf[k], 0, want[k], c->stream) != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "hipMemsetAsync failed");
            }
    }
    return 0;
}

// the buffers of a run, and its source table in HBM
int ensure_run(ethcnn_replay* p, int run, const Need& nd) {
    ethcnn_ctx* c = p->c;
    const Run& r = p->plan.runs[(size_t)run];
    char what[96];
    std::snprintf(what, sizeof what, "run %d (%lld frames of %lld CTUs)", run, (long long)r.F, (long long)r.nctu);
    if (int rc = ensure_buffers(p, nd, what)) return rc;
    c->done_armed = 0;
    if (p->src_run != run) {
        p->src_run = -1;
        const hipError_t e = hipMemcpyAsync(p->d_src, p->plan.src.data() + r.src_at, nd.src, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "upload of the source table: %s", hipGetErrorString(e));
        p->src_run = run;
    }
    return 0;
}

int begin_open(ethcnn_replay* p) {
    if (hipSetDevice(p->c->device) != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "hipSetDevice(%d) failed", p->c->device);
    close_all(p);  // an object that is opened again starts over
    return 0;
}
}  // namespace

extern "C" int ethcnn_replay_plan(const uint8_t* records, size_t nbytes, ethcnn_replay_run* runs_out, int max_runs, int* nruns_out, int64_t* src_out,
                                  char* err, size_t errcap) {
    auto say = [&](int code, const std::string& s) {
        if (err && errcap) std::snprintf(err, errcap, "%s", s.c_str());
        return code;
    };
    if (err && errcap) err[0] = 0;
    if (nruns_out) *nruns_out = 0;
    if ((!records && nbytes) || max_runs < 0) return say(ETHCNN_ERR_ARG, "null records or a negative run capacity");
    if (nbytes == 0 || nbytes % kRec) return say(ETHCNN_ERR_FORMAT, std::to_string(nbytes) + " bytes is not a whole number of 16516-byte records");
    const int64_t n = (int64_t)(nbytes / kRec);
    std::vector<Header> hdr((size_t)n);
    for (int64_t i = 0; i < n; ++i) hdr[(size_t)i] = header_of(records + (size_t)i * kRec);
    Plan pl;
    std::string why;
    if (!plan(hdr.data(), n, &pl, &why)) return say(ETHCNN_ERR_FORMAT, why);
    if (nruns_out) *nruns_out = (int)pl.runs.size();
    if (runs_out)
        for (int k = 0; k < (int)pl.runs.size() && k < max_runs; ++k) fill_run(pl.runs[(size_t)k], runs_out + k);
    if (src_out) std::copy(pl.src.begin(), pl.src.end(), src_out);
    return ETHCNN_OK;
}

extern "C" int ethcnn_replay_uncut_device(ethcnn_ctx* c, const uint8_t* d_records, int64_t nrecords, const int64_t* d_src, int64_t nframes, int R, int C,
                                          int slot, uint8_t* d_resi, uint8_t* d_labels) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!d_records || !d_src || !d_resi || !d_labels) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_replay_uncut_device: null buffer");
    if ((uintptr_t)d_records % 4 || (uintptr_t)d_src % 8 || (uintptr_t)d_resi % 16 || (uintptr_t)d_labels % 4)
        return set_err(c, ETHCNN_ERR_ARG, "ethcnn_replay_uncut_device: records and labels are 4-byte, the table 8-byte and the residual planes 16-byte aligned");
    if (slot < 0 || slot > 3) return set_err(c, ETHCNN_ERR_ARG, "QP slot %d outside 0..3", slot);
    if (nrecords < 0 || nframes < 0 || R <= 0 || C <= 0 || R > 1023 || C > 1023 || (int64_t)R * C > kMaxCtus)
        return set_err(c, ETHCNN_ERR_ARG, "ethcnn_replay_uncut_device: bad counts (%lld records, %lld frames of %d x %d CTUs)", (long long)nrecords,
                       (long long)nframes, R, C);
    if (nframes == 0) return ETHCNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;  // the context's completion word does not cover this launch
    launch_uncut(c->stream, d_records, (long)nrecords, d_src, (long)nframes, R, C, slot, d_resi, d_labels, cus_of(c));
    HIPCHK(c, hipGetLastError());
    return ETHCNN_OK;
}

extern "C" int ethcnn_replay_create(ethcnn_ctx* c, uint64_t max_bytes, ethcnn_replay** out) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "null output pointer");
    *out = nullptr;
    ethcnn_replay* p = new (std::nothrow) ethcnn_replay;
    if (!p) return set_err(c, ETHCNN_ERR_NOMEM, "out of memory");
    p->c = c;
    p->max_bytes = max_bytes;
    *out = p;
    return ETHCNN_OK;
}

extern "C" void ethcnn_replay_destroy(ethcnn_replay* p) {
    if (!p) return;
    (void)hipSetDevice(p->c->device);
    close_all(p);
    delete p;
}

extern "C" const char* ethcnn_replay_last_error(const ethcnn_replay* p) { return p ? p->err.c_str() : "replay object is NULL"; }

extern "C" int ethcnn_replay_open_records(ethcnn_replay* p, const uint8_t* records, size_t nbytes) {
    if (!p) return ETHCNN_ERR_ARG;
    if (!records && nbytes) return rerr(p, ETHCNN_ERR_ARG, "null records");
    if (int rc = begin_open(p)) return rc;
    if (nbytes == 0 || nbytes % kRec) return rerr(p, ETHCNN_ERR_FORMAT, "%zu bytes is not a whole number of %d-byte records", nbytes, kRec);
    const int64_t n = (int64_t)(nbytes / kRec);
    Plan pl;
    {
        std::vector<Header> hdr((size_t)n);
        for (int64_t i = 0; i < n; ++i) hdr[(size_t)i] = header_of(records + (size_t)i * kRec);
        std::string why;
        if (!plan(hdr.data(), n, &pl, &why)) return rerr(p, ETHCNN_ERR_FORMAT, "%s", why.c_str());
    }
    if (p->max_bytes && nbytes > p->max_bytes)
        return rerr(p, ETHCNN_ERR_NOMEM, "the copy of %lld records needs %zu bytes, above the object's limit of %llu", (long long)n, nbytes,
                    (unsigned long long)p->max_bytes);
    ethcnn_ctx* c = p->c;
    uint8_t* up = nullptr;
    if (hipMalloc((void**)&up, nbytes) != hipSuccess) {
        (void)hipGetLastError();
        return rerr(p, ETHCNN_ERR_NOMEM, "the copy of %lld records: %zu bytes do not fit in device memory", (long long)n, nbytes);
    }
    hipError_t e = hipSuccess;
    for (size_t at = 0; at < nbytes && e == hipSuccess; at += kIoBytes)
        e = hipMemcpyAsync(up + at, records + at, std::min(kIoBytes, nbytes - at), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the caller's memory is free when this returns
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(up);
        return rerr(p, ETHCNN_ERR_DEVICE, "upload of the records: %s", hipGetErrorString(e));
    }
    p->own = up;
    p->rec = up;
    p->nrec = n;
    p->plan = std::move(pl);
    return ETHCNN_OK;
}

extern "C" int ethcnn_replay_open_set(ethcnn_replay* p, ethcnn_samples* set) {
    if (!p) return ETHCNN_ERR_ARG;
    if (!set) return rerr(p, ETHCNN_ERR_ARG, "null sample set");
    if (int rc = begin_open(p)) return rc;
    if (set->kind != ethcnn::samples::kKindInter)
        return rerr(p, ETHCNN_ERR_FORMAT, "a set of %d-byte All-Intra records has no header and no residual: a replay takes an inter set", set->record_bytes());
    if (!set->built || set->count == 0 || !set->data) return rerr(p, ETHCNN_ERR_FORMAT, "the sample set is not built or holds no records");
    if (set->c != p->c) return rerr(p, ETHCNN_ERR_ARG, "the sample set lives on another context");
    ethcnn_ctx* c = p->c;
    const int64_t n = set->count;
    // the headers leave HBM as 20 bytes a record (scratch that is gone before anything else is allocated, outside the memory sum)
    Header* d_hdr = nullptr;
    if (hipMalloc((void**)&d_hdr, (size_t)n * sizeof(Header)) != hipSuccess) {
        (void)hipGetLastError();
        return rerr(p, ETHCNN_ERR_NOMEM, "%zu bytes of record headers do not fit in device memory", (size_t)n * sizeof(Header));
    }
    std::vector<Header> hdr((size_t)n);
    c->done_armed = 0;
    launch_headers(c->stream, set->data, (long)n, d_hdr, cus_of(c));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(hdr.data(), d_hdr, (size_t)n * sizeof(Header), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_hdr);
    if (e != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "record headers: %s", hipGetErrorString(e));
    Plan pl;
    std::string why;
    if (!plan(hdr.data(), n, &pl, &why)) return rerr(p, ETHCNN_ERR_FORMAT, "%s", why.c_str());
    p->rec = set->data;
    p->nrec = n;
    p->plan = std::move(pl);
    return ETHCNN_OK;
}

extern "C" int ethcnn_replay_run_count(const ethcnn_replay* p) { return p ? (int)p->plan.runs.size() : ETHCNN_ERR_ARG; }

extern "C" int ethcnn_replay_run_info(ethcnn_replay* p, int run, ethcnn_replay_run* out) {
    if (!p) return ETHCNN_ERR_ARG;
    if (!out) return rerr(p, ETHCNN_ERR_ARG, "null output pointer");
    if (int rc = check_run(p, run, 0)) return rc;
    fill_run(p->plan.runs[(size_t)run], out);
    return ETHCNN_OK;
}

extern "C" int ethcnn_replay_set_chunk_frames(ethcnn_replay* p, int frames) {
    if (!p) return ETHCNN_ERR_ARG;
    if (frames < 0) return rerr(p, ETHCNN_ERR_ARG, "ethcnn_replay_set_chunk_frames: %d frames", frames);
    p->chunk = frames;
    return ETHCNN_OK;
}

extern "C" int64_t ethcnn_replay_run_bytes(ethcnn_replay* p, int run, int own_probs, int own_labels) {
    if (!p) return ETHCNN_ERR_ARG;
    if (int rc = check_run(p, run, 0)) return rc;
    return (int64_t)need_of(p, p->plan.runs[(size_t)run], own_probs != 0, own_labels != 0).total();
}

extern "C" int ethcnn_replay_run_device(ethcnn_replay* p, int run, int slot, float* d_probs, uint8_t* d_labels) {
    if (!p) return ETHCNN_ERR_ARG;
    if (int rc = check_run(p, run, slot)) return rc;
    if (((uintptr_t)d_probs | (uintptr_t)d_labels) % 4) return rerr(p, ETHCNN_ERR_ARG, "output buffers are 4-byte aligned");
    ethcnn_ctx* c = p->c;
    const Run& r = p->plan.runs[(size_t)run];
    if (!c->have_weights) return rerr(p, ETHCNN_ERR_NOWEIGHTS, "the context has no residual CNN loaded (ethcnn_load_checkpoint / ethcnn_load_blob)");
    if (!c->have_lstm)
        return rerr(p, ETHCNN_ERR_NOWEIGHTS, "the context has no ETH-LSTM bundle loaded for QP %d of slot %d (ethcnn_load_lstm_checkpoint / ethcnn_load_lstm_blob)", r.qp[slot], slot);
    if (hipSetDevice(c->device) != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "hipSetDevice(%d) failed", c->device);
    if (int rc = ensure_run(p, run, need_of(p, r, d_probs == nullptr, d_labels == nullptr))) return rc;
    hipError_t e = hipSuccess;
    float* probs = d_probs ? d_probs : p->d_probs;
    uint8_t* labels = d_labels ? d_labels : p->d_labels;
    const int64_t Fc = chunk_frames(p, r);
    const int W = 64 * r.C, H = 64 * r.R;
    for (int64_t at = 0; at < r.F; at += Fc) {
        const int nf = (int)std::min<int64_t>(Fc, r.F - at);
        c->done_armed = 0;
        launch_uncut(c->stream, p->rec, (long)p->nrec, p->d_src + at * r.nctu, nf, r.R, r.C, slot, p->d_resi, labels + at * r.nctu * 16, cus_of(c));
        e = hipGetLastError();
        if (e != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "uncut: %s", hipGetErrorString(e));
        // the first chunk starts from zeros (the object's zero state when its frame number is above 1); the following ones from the
        // state the call before left resident
        const int rc = ethcnn_ldp_sequence_device(c, p->d_resi, W, H, W, (ptrdiff_t)W * H, nf, r.qp[slot], (int)(r.f0 + (uint32_t)at),
                                                  at == 0 && r.f0 > 1 ? p->d_zero : nullptr, probs + at * r.nctu * kNOut);
        if (rc) return rerr(p, rc, "run %d, frames %lld..%lld: %s", run, (long long)(r.f0 + at), (long long)(r.f0 + at + nf - 1), ethcnn_last_error(c));
    }
    return ETHCNN_OK;
}

extern "C" int64_t ethcnn_replay_run_group_bytes(ethcnn_replay* p, int run, int nslots) {
    if (!p) return ETHCNN_ERR_ARG;
    if (int rc = check_run(p, run, 0)) return rc;
    if (nslots < 1 || nslots > kLstmSeqGroupMax) return rerr(p, ETHCNN_ERR_ARG, "%d slots (1..%d)", nslots, kLstmSeqGroupMax);
    return (int64_t)need_of(p, p->plan.runs[(size_t)run], false, false, nslots).total();
}

extern "C" int ethcnn_replay_run_group_device(ethcnn_replay* p, int run, int nslots, const int* slots, ethcnn_ldp_group* grp, float* const* d_probs,
                                              uint8_t* const* d_labels) {
    if (!p) return ETHCNN_ERR_ARG;
    if (int rc = check_run(p, run, 0)) return rc;
    if (!grp || !slots || !d_probs || !d_labels) return rerr(p, ETHCNN_ERR_ARG, "ethcnn_replay_run_group_device: null pointer");
    if (grp->c != p->c) return rerr(p, ETHCNN_ERR_ARG, "the group lives on another context");
    if (nslots != grp->nb) return rerr(p, ETHCNN_ERR_ARG, "%d slots for a group of %d members", nslots, grp->nb);
    for (int j = 0; j < nslots; ++j) {
        if (int rc = check_run(p, run, slots[j])) return rc;
        if (!d_probs[j] || !d_labels[j]) return rerr(p, ETHCNN_ERR_ARG, "ethcnn_replay_run_group_device: null output buffer (slot %d)", slots[j]);
        if (((uintptr_t)d_probs[j] | (uintptr_t)d_labels[j]) % 4) return rerr(p, ETHCNN_ERR_ARG, "output buffers are 4-byte aligned");
    }
    ethcnn_ctx* c = p->c;
    const Run& r = p->plan.runs[(size_t)run];
    if (!c->have_weights) return rerr(p, ETHCNN_ERR_NOWEIGHTS, "the context has no residual CNN loaded (ethcnn_load_checkpoint / ethcnn_load_blob)");
    for (int j = 0; j < nslots; ++j)
        if (!grp->b[j].have)
            return rerr(p, ETHCNN_ERR_NOWEIGHTS, "member %d of the group has no ETH-LSTM bundle loaded for QP %d of slot %d", j, r.qp[slots[j]], slots[j]);
    if (hipSetDevice(c->device) != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "hipSetDevice(%d) failed", c->device);
    if (int rc = ensure_run(p, run, need_of(p, r, false, false, nslots))) return rc;
    const int64_t Fc = chunk_frames(p, r);
    const int W = 64 * r.C, H = 64 * r.R;
    const size_t plane_chunk = (size_t)(Fc * r.nctu) * 4096;  // slot j's planes of a chunk start at j * plane_chunk
    const uint8_t* luma[kLstmSeqGroupMax];
    const float* zero[kLstmSeqGroupMax];
    float* probs[kLstmSeqGroupMax];
    int qp[kLstmSeqGroupMax];
    for (int j = 0; j < nslots; ++j) luma[j] = p->d_resi + (size_t)j * plane_chunk, zero[j] = p->d_zero, qp[j] = r.qp[slots[j]];
    for (int64_t at = 0; at < r.F; at += Fc) {
        const int nf = (int)std::min<int64_t>(Fc, r.F - at);
        c->done_armed = 0;
        for (int j = 0; j < nslots; ++j) {
            launch_uncut(c->stream, p->rec, (long)p->nrec, p->d_src + at * r.nctu, nf, r.R, r.C, slots[j], p->d_resi + (size_t)j * plane_chunk,
                         d_labels[j] + at * r.nctu * 16, cus_of(c));
            probs[j] = d_probs[j] + at * r.nctu * kNOut;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "uncut: %s", hipGetErrorString(e));
        // the first chunk starts from zeros (the object's zero state when its frame number is above 1); the following ones from the
        // states the call before left resident in the group
        const int rc = ethcnn_ldp_group_sequence_device(grp, luma, W, H, W, (ptrdiff_t)W * H, nf, qp, (int)(r.f0 + (uint32_t)at),
                                                        at == 0 && r.f0 > 1 ? zero : nullptr, probs);
        if (rc) return rerr(p, rc, "run %d, frames %lld..%lld: %s", run, (long long)(r.f0 + at), (long long)(r.f0 + at + nf - 1), ethcnn_ldp_group_last_error(grp));
    }
    return ETHCNN_OK;
}

extern "C" int ethcnn_replay_feed_calib(ethcnn_replay* p, int run, int slot, ethcnn_calib* cal) {
    if (!p) return ETHCNN_ERR_ARG;
    if (!cal) return rerr(p, ETHCNN_ERR_ARG, "null calibrator");
    if (cal->c != p->c) return rerr(p, ETHCNN_ERR_ARG, "the calibrator lives on another context");
    if (int rc = ethcnn_replay_run_device(p, run, slot, nullptr, nullptr)) return rc;
    const Run& r = p->plan.runs[(size_t)run];
    const int rc = ethcnn_calib_add_frames_device(cal, p->d_probs, p->d_labels, 64 * r.C, 64 * r.R, r.F, 0);
    return rc ? rerr(p, rc, "run %d: %s", run, ethcnn_last_error(p->c)) : ETHCNN_OK;
}

extern "C" int ethcnn_replay_feed_sim(ethcnn_replay* p, int run, int slot, ethcnn_sim* sim) {
    if (!p) return ETHCNN_ERR_ARG;
    if (!sim) return rerr(p, ETHCNN_ERR_ARG, "null simulator");
    if (sim->c != p->c) return rerr(p, ETHCNN_ERR_ARG, "the simulator lives on another context");
    if (int rc = ethcnn_replay_run_device(p, run, slot, nullptr, nullptr)) return rc;
    const Run& r = p->plan.runs[(size_t)run];
    const int rc = ethcnn_sim_add_frames_device(sim, p->d_probs, p->d_labels, 64 * r.C, 64 * r.R, r.F, 0);
    return rc ? rerr(p, rc, "run %d: %s", run, ethcnn_last_error(p->c)) : ETHCNN_OK;
}

// ---- several runs through an ethcnn_ldp_batch (config #5 offline, batch form): item j = run runs[j] at slot slots[j] with bundle
// bundles[j].  The items go to the batch in the order of their lengths, longest first (stable), so that the items which still have
// frames are always the first ones of the list and every item keeps its sequence index -- and with it its resident state -- from
// chunk to chunk.  No result depends on that order.
namespace {
struct BatchLayout {
    int order[kLstmSeqBatchMax];        // position in the batch call -> item
    size_t plane_at[kLstmSeqBatchMax];  // bytes into d_resi, by item
    size_t src_at[kLstmSeqBatchMax];    // entries into d_src, by item
    size_t out_at[kLstmSeqBatchMax];    // CTU-frames into the object's own probabilities and labels, by item
    int64_t Fc, longest;
    Need nd;
};

int batch_layout(ethcnn_replay* p, ethcnn_ldp_batch* b, int nitems, const int* runs, bool own_out, BatchLayout* L) {
    if (p->plan.runs.empty()) return rerr(p, ETHCNN_ERR_ARG, "nothing is open (ethcnn_replay_open_set / ethcnn_replay_open_records)");
    if (!b || !runs) return rerr(p, ETHCNN_ERR_ARG, "ethcnn_replay_batch: null pointer");
    if (b->c != p->c) return rerr(p, ETHCNN_ERR_ARG, "the batch lives on another context");
    if (nitems < 1 || nitems > kLstmSeqBatchMax) return rerr(p, ETHCNN_ERR_ARG, "%d items (1..%d)", nitems, kLstmSeqBatchMax);
    int64_t sum = 0;
    for (int j = 0; j < nitems; ++j) {
        if (int rc = check_run(p, runs[j], 0)) return rc;
        sum += p->plan.runs[(size_t)runs[j]].nctu;
    }
    L->Fc = p->chunk > 0 ? (int64_t)p->chunk : std::max<int64_t>(1, kChunkBytes / (sum * 4096));
    L->longest = 0;
    Need& n = L->nd;
    n.rec = p->own ? (size_t)p->nrec * kRec : 0;
    n.resi = n.src = n.probs = n.labels = n.zero = 0;
    size_t ctu_frames = 0;
    for (int j = 0; j < nitems; ++j) {
        const Run& r = p->plan.runs[(size_t)runs[j]];
        L->order[j] = j;
        L->plane_at[j] = n.resi, L->src_at[j] = ctu_frames, L->out_at[j] = ctu_frames;
        n.resi += (size_t)(std::min<int64_t>(r.F, L->Fc) * r.nctu) * 4096;
        ctu_frames += (size_t)(r.F * r.nctu);
        if (r.f0 > 1) n.zero = std::max(n.zero, (size_t)r.nctu * 2 * kNVec * 4);
        L->longest = std::max(L->longest, r.F);
    }
    n.src = ctu_frames * 8;
    if (own_out) n.probs = ctu_frames * kNOut * 4, n.labels = ctu_frames * 16;
    std::stable_sort(L->order, L->order + nitems, [&](int x, int y) { return p->plan.runs[(size_t)runs[x]].F > p->plan.runs[(size_t)runs[y]].F; });
    return 0;
}

// d_probs / d_labels null: into the object's own buffers at out_at
int batch_replay(ethcnn_replay* p, ethcnn_ldp_batch* b, int nitems, const int* runs, const int* slots, const int* bundles, float* const* d_probs,
                 uint8_t* const* d_labels, BatchLayout* L) {
    const bool own_out = d_probs == nullptr;
    if (int rc = batch_layout(p, b, nitems, runs, own_out, L)) return rc;
    if (!slots || !bundles) return rerr(p, ETHCNN_ERR_ARG, "ethcnn_replay_batch: null pointer");
    ethcnn_ctx* c = p->c;
    if (!c->have_weights) return rerr(p, ETHCNN_ERR_NOWEIGHTS, "the context has no residual CNN loaded (ethcnn_load_checkpoint / ethcnn_load_blob)");
    for (int j = 0; j < nitems; ++j) {
        if (int rc = check_run(p, runs[j], slots[j])) return rc;
        if (bundles[j] < 0 || bundles[j] >= b->nb || !b->b[bundles[j]].have)
            return rerr(p, ETHCNN_ERR_NOWEIGHTS, "item %d: bundle %d of the batch holds no ETH-LSTM bundle for QP %d of slot %d", j, bundles[j],
                        p->plan.runs[(size_t)runs[j]].qp[slots[j]], slots[j]);
        if (!own_out) {
            if (!d_labels || !d_probs[j] || !d_labels[j]) return rerr(p, ETHCNN_ERR_ARG, "ethcnn_replay_batch_device: null output buffer (item %d)", j);
            if (((uintptr_t)d_probs[j] | (uintptr_t)d_labels[j]) % 4) return rerr(p, ETHCNN_ERR_ARG, "output buffers are 4-byte aligned");
        }
    }
    if (hipSetDevice(c->device) != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "hipSetDevice(%d) failed", c->device);
    char what[96];
    std::snprintf(what, sizeof what, "a batch of %d runs (chunks of %lld frames)", nitems, (long long)L->Fc);
    if (int rc = ensure_buffers(p, L->nd, what)) return rc;
    c->done_armed = 0;
    p->src_run = -1;  // the table buffer holds the items' tables, one behind the other
    for (int j = 0; j < nitems; ++j) {
        const Run& r = p->plan.runs[(size_t)runs[j]];
        const hipError_t e = hipMemcpyAsync(p->d_src + L->src_at[j], p->plan.src.data() + r.src_at, (size_t)(r.F * r.nctu) * 8, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "upload of the source table: %s", hipGetErrorString(e));
    }
    for (int64_t at = 0; at < L->longest; at += L->Fc) {
        ethcnn_ldp_batch_seq seqs[kLstmSeqBatchMax];
        int k = 0;
        for (; k < nitems; ++k) {
            const int j = L->order[k];
            const Run& r = p->plan.runs[(size_t)runs[j]];
            if (at >= r.F) break;  // (sorted by length: everything behind it has ended as well)
            const int nf = (int)std::min<int64_t>(L->Fc, r.F - at), W = 64 * r.C, H = 64 * r.R;
            float* const probs = own_out ? p->d_probs + L->out_at[j] * kNOut : d_probs[j];
            uint8_t* const labels = own_out ? p->d_labels + L->out_at[j] * 16 : d_labels[j];
            launch_uncut(c->stream, p->rec, (long)p->nrec, p->d_src + L->src_at[j] + at * r.nctu, nf, r.R, r.C, slots[j], p->d_resi + L->plane_at[j],
                         labels + at * r.nctu * 16, cus_of(c));
            // the first chunk starts from zeros (the object's zero state when the frame number is above 1); the following ones from the
            // state the call before left resident at this position of the batch
            seqs[k] = {p->d_resi + L->plane_at[j], W, H, (ptrdiff_t)W, (ptrdiff_t)W * H, nf, r.qp[slots[j]], (int)(r.f0 + (uint32_t)at), bundles[j],
                       at == 0 && r.f0 > 1 ? p->d_zero : nullptr, probs + at * r.nctu * kNOut};
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return rerr(p, ETHCNN_ERR_DEVICE, "uncut: %s", hipGetErrorString(e));
        const int rc = ethcnn_ldp_batch_run_device(b, seqs, k);
        if (rc) return rerr(p, rc, "batch of %d runs, frames %lld.. of each: %s", nitems, (long long)at, ethcnn_ldp_batch_last_error(b));
    }
    return ETHCNN_OK;
}

template <typename Add>
int batch_feed(ethcnn_replay* p, ethcnn_ldp_batch* b, int nitems, const int* runs, const int* slots, const int* bundles, Add add) {
    // the consumers take UNGATED probabilities (open gates on the context): a pair of an index's own would gate them all the same
    if (b)
        for (int j = 0; j < kLstmSeqBatchMax; ++j)
            if (b->s[j].own_gates)
                return rerr(p, ETHCNN_ERR_ARG, "sequence index %d of the batch holds thresholds of its own (%g, %g): a feed needs open gates (ethcnn_ldp_clear_thresholds_batch)",
                            j, (double)b->s[j].thr1, (double)b->s[j].thr2);
    BatchLayout L;
    if (int rc = batch_replay(p, b, nitems, runs, slots, bundles, nullptr, nullptr, &L)) return rc;
    for (int j = 0; j < nitems; ++j) {  // in list order: the consumer ends as the per-run feeds in that order leave it
        const Run& r = p->plan.runs[(size_t)runs[j]];
        const int rc = add(p->d_probs + L.out_at[j] * kNOut, p->d_labels + L.out_at[j] * 16, 64 * r.C, 64 * r.R, r.F);
        if (rc) return rerr(p, rc, "run %d: %s", runs[j], ethcnn_last_error(p->c));
    }
    return ETHCNN_OK;
}
}  // namespace

extern "C" int64_t ethcnn_replay_batch_bytes(ethcnn_replay* p, ethcnn_ldp_batch* b, int nitems, const int* runs) {
    if (!p) return ETHCNN_ERR_ARG;
    BatchLayout L;
    if (int rc = batch_layout(p, b, nitems, runs, false, &L)) return rc;
    return (int64_t)L.nd.total();
}

extern "C" int ethcnn_replay_batch_device(ethcnn_replay* p, ethcnn_ldp_batch* b, int nitems, const int* runs, const int* slots, const int* bundles,
                                          float* const* d_probs, uint8_t* const* d_labels) {
    if (!p) return ETHCNN_ERR_ARG;
    if (!d_probs || !d_labels) return rerr(p, ETHCNN_ERR_ARG, "ethcnn_replay_batch_device: null pointer");
    BatchLayout L;
    return batch_replay(p, b, nitems, runs, slots, bundles, d_probs, d_labels, &L);
}

extern "C" int ethcnn_replay_batch_feed_calib(ethcnn_replay* p, ethcnn_ldp_batch* b, int nitems, const int* runs, const int* slots, const int* bundles,
                                              ethcnn_calib* cal) {
    if (!p) return ETHCNN_ERR_ARG;
    if (!cal) return rerr(p, ETHCNN_ERR_ARG, "null calibrator");
    if (cal->c != p->c) return rerr(p, ETHCNN_ERR_ARG, "the calibrator lives on another context");
    return batch_feed(p, b, nitems, runs, slots, bundles, [&](const float* probs, const uint8_t* labels, int w, int h, int64_t F) {
        return ethcnn_calib_add_frames_device(cal, probs, labels, w, h, F, 0);
    });
}

extern "C" int ethcnn_replay_batch_feed_sim(ethcnn_replay* p, ethcnn_ldp_batch* b, int nitems, const int* runs, const int* slots, const int* bundles,
                                            ethcnn_sim* sim) {
    if (!p) return ETHCNN_ERR_ARG;
    if (!sim) return rerr(p, ETHCNN_ERR_ARG, "null simulator");
    if (sim->c != p->c) return rerr(p, ETHCNN_ERR_ARG, "the simulator lives on another context");
    return batch_feed(p, b, nitems, runs, slots, bundles, [&](const float* probs, const uint8_t* labels, int w, int h, int64_t F) {
        return ethcnn_sim_add_frames_device(sim, probs, labels, w, h, F, 0);
    });
}
