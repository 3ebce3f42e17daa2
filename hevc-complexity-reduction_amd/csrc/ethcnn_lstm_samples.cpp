// ethcnn_lstm_samples.cpp -- host side of the ETH-LSTM sample sets (include/ethcnn.h "ETH-LSTM sample sets"): the selection, the memory
// plan, the build loop (slot -> chunks of records -> repack + residual CNN -> gather), read-back and the file writer.  The job of
// get_LSTM_input.py's build_samples, with the records, the vectors and the samples in HBM (kernels: ethcnn_lstm_samples_kernels.hip).
#include "ethcnn_ctx.h"
#include "ethcnn_lstm_samples.h"
#include "ethcnn_samples.h"

using namespace ethcnn::lstm_samples;

namespace {
constexpr size_t kIoBytes = 64u << 20;  // upload / read-back / file-writer piece

int lerr(ethcnn_lstm_samples* s, int code, const char* fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    s->err = buf;
    return code;
}

// device allocations of one build: all of them go when the build leaves, except the one it hands over
struct Arena {
    std::vector<void*> p;
    ~Arena() {
        for (void* q : p)
            if (q) (void)hipFree(q);
    }
    void* get(size_t bytes) {
        void* q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 4) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        p.push_back(q);
        return q;
    }
    void release(void* q) {
        for (void*& x : p)
            if (x == q) x = nullptr;
    }
};

void drop(ethcnn_lstm_samples* s) {
    if (s->data) {
        (void)hipStreamSynchronize(s->c->stream);
        (void)hipFree(s->data);
    }
    s->data = nullptr;
    s->count = s->skipped = 0;
    s->built = false;
}

// the build proper.  `d_rec`: nrec records in HBM (NULL: `h_rec` is uploaded first, as part of the working buffers); `pl`: their plan.
int build(ethcnn_lstm_samples* s, const uint8_t* d_rec, const uint8_t* h_rec, int64_t nrec, const Plan& pl) {
    ethcnn_ctx* c = s->c;
    const int64_t m = (int64_t)pl.heads.size();
    const unsigned long long out_bytes = (unsigned long long)m * s->nslots * kRecOut;
    const int chunk = (int)std::min<int64_t>(s->chunk, (nrec + kTileCols - 1) / kTileCols * kTileCols);
    const unsigned long long vec_bytes = (unsigned long long)((nrec + kTileCols - 1) / kTileCols * kTileCols) * kVec * 4,
                             pic_bytes = (unsigned long long)chunk * 4096, plan_bytes = (unsigned long long)m * 16,
                             rec_bytes = d_rec ? 0ull : (unsigned long long)nrec * kRecIn,
                             total = out_bytes + vec_bytes + pic_bytes + plan_bytes + rec_bytes;
    if (s->max_bytes && total > s->max_bytes)
        return lerr(s, ETHCNN_ERR_NOMEM, "%lld samples of %lld records need %llu bytes (%llu of samples, %llu of working buffers), above the set's limit of %llu",
                    (long long)(m * s->nslots), (long long)nrec, total, out_bytes, total - out_bytes, (unsigned long long)s->max_bytes);
    s->skipped = pl.skipped;
    if (m == 0) {
        s->built = true;
        return ETHCNN_OK;
    }
    Arena ar;
    auto nomem = [&]() {
        s->skipped = 0;
        return lerr(s, ETHCNN_ERR_NOMEM, "%lld samples of %lld records: %llu bytes do not fit in device memory", (long long)(m * s->nslots),
                    (long long)nrec, total);
    };
    uint8_t* out = (uint8_t*)ar.get((size_t)out_bytes);
    float* vec = out ? (float*)ar.get((size_t)vec_bytes) : nullptr;
    uint8_t* pic = vec ? (uint8_t*)ar.get((size_t)pic_bytes) : nullptr;
    int64_t* d_plan = pic ? (int64_t*)ar.get((size_t)plan_bytes) : nullptr;
    if (!d_plan) return nomem();
    hipError_t e = hipSuccess;
    if (!d_rec) {
        uint8_t* up = (uint8_t*)ar.get((size_t)rec_bytes);
        if (!up) return nomem();
        for (size_t at = 0; at < (size_t)rec_bytes && e == hipSuccess; at += kIoBytes)
            e = hipMemcpyAsync(up + at, h_rec + at, std::min(kIoBytes, (size_t)rec_bytes - at), hipMemcpyHostToDevice, c->stream);
        d_rec = up;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(d_plan, pl.heads.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_plan + m, pl.strides.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream);
    const int cus = c->cus > 0 ? c->cus : 256;
    int rc = 0;
    for (int i = 0; i < s->nslots && e == hipSuccess && !rc; ++i) {
        for (int64_t r0 = 0; r0 < nrec && e == hipSuccess && !rc; r0 += chunk) {
            const int n = (int)std::min<int64_t>(chunk, nrec - r0), rows = (n + kTileCols - 1) / kTileCols;
            c->done_armed = 0;  // the context's completion word does not cover this launch
            launch_repack(c->stream, d_rec, (long)nrec, (long)r0, n, s->slots[i], pic, cus);
            e = hipGetLastError();
            if (e == hipSuccess && (rc = ethcnn_resi_vectors_device(c, pic, kPitch, rows * 64, kPitch, vec + (size_t)r0 * kVec)) != 0)
                lerr(s, rc, "build: residual CNN on records %lld..%lld: %s", (long long)r0, (long long)(r0 + n - 1), ethcnn_last_error(c));
        }
        if (e != hipSuccess || rc) break;
        c->done_armed = 0;
        launch_sample_gather(c->stream, d_rec, vec, d_plan, d_plan + m, (long)m, s->slots[i], out + (size_t)i * (size_t)m * kRecOut, cus);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(c->stream);  // (also before the working buffers go, whatever happened)
    if (e == hipSuccess) e = e2;
    if (!rc && e != hipSuccess) rc = lerr(s, ETHCNN_ERR_DEVICE, "build: %s", hipGetErrorString(e));
    if (rc) {
        s->skipped = 0;
        return rc;
    }
    ar.release(out);
    s->data = out;
    s->count = m * s->nslots;
    s->built = true;
    return ETHCNN_OK;
}

int begin(ethcnn_lstm_samples* s) {
    ethcnn_ctx* c = s->c;
    if (hipSetDevice(c->device) != hipSuccess) return lerr(s, ETHCNN_ERR_DEVICE, "hipSetDevice(%d) failed", c->device);
    drop(s);  // a set that is built again starts over
    if (!c->have_weights) return lerr(s, ETHCNN_ERR_NOWEIGHTS, "the context has no residual CNN loaded (ethcnn_load_checkpoint / ethcnn_load_blob)");
    return 0;
}
}  // namespace

extern "C" int ethcnn_lstm_samples_plan(const uint8_t* records, size_t nbytes, int64_t* heads, int64_t* strides, int64_t* nheads,
                                        int64_t* skipped) {
    if (!records && nbytes) return ETHCNN_ERR_ARG;
    if (nbytes == 0 || nbytes % kRecIn) return ETHCNN_ERR_FORMAT;
    Plan pl;
    plan((int64_t)(nbytes / kRecIn), [&](int64_t r) { return header_of(records + (size_t)r * kRecIn); }, &pl);
    if (heads) std::copy(pl.heads.begin(), pl.heads.end(), heads);
    if (strides) std::copy(pl.strides.begin(), pl.strides.end(), strides);
    if (nheads) *nheads = (int64_t)pl.heads.size();
    if (skipped) *skipped = pl.skipped;
    return ETHCNN_OK;
}

extern "C" int ethcnn_lstm_samples_create(ethcnn_ctx* c, const int* slots, int nslots, int chunk_ctus, uint64_t max_bytes,
                                          ethcnn_lstm_samples** out) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!out) return set_err(c, ETHCNN_ERR_ARG, "null output pointer");
    *out = nullptr;
    if (nslots < 0 || nslots > 4 || (nslots > 0 && !slots)) return set_err(c, ETHCNN_ERR_ARG, "the slot list must hold 0..4 entries, got %d", nslots);
    bool on[4] = {false, false, false, false};
    for (int i = 0; i < nslots; ++i) {
        if (slots[i] < 0 || slots[i] > 3) return set_err(c, ETHCNN_ERR_ARG, "QP slot %d outside 0..3", slots[i]);
        if (on[slots[i]]) return set_err(c, ETHCNN_ERR_ARG, "QP slot %d is listed twice", slots[i]);
        on[slots[i]] = true;
    }
    const int cap = c->max_ctus / kTileCols * kTileCols;
    if (chunk_ctus < 0 || chunk_ctus % kTileCols || chunk_ctus > cap)
        return set_err(c, ETHCNN_ERR_ARG, "chunk_ctus %d: 0 (default) or a multiple of %d up to the context's max_ctus_per_pass (%d)", chunk_ctus,
                       kTileCols, cap);
    ethcnn_lstm_samples* s = new (std::nothrow) ethcnn_lstm_samples;
    if (!s) return set_err(c, ETHCNN_ERR_NOMEM, "out of memory");
    s->c = c;
    if (nslots) {
        s->nslots = 0;
        for (int q = 0; q < 4; ++q)
            if (on[q]) s->slots[s->nslots++] = q;
    }
    s->chunk = chunk_ctus ? chunk_ctus : std::min(kDefaultChunk, cap);
    s->max_bytes = max_bytes;
    *out = s;
    return ETHCNN_OK;
}

extern "C" void ethcnn_lstm_samples_destroy(ethcnn_lstm_samples* s) {
    if (!s) return;
    if (s->data) {
        (void)hipSetDevice(s->c->device);
        drop(s);
    }
    delete s;
}

extern "C" const char* ethcnn_lstm_samples_last_error(const ethcnn_lstm_samples* s) { return s ? s->err.c_str() : "sample set is NULL"; }
extern "C" int64_t ethcnn_lstm_samples_count(const ethcnn_lstm_samples* s) { return s ? s->count : ETHCNN_ERR_ARG; }
extern "C" int64_t ethcnn_lstm_samples_skipped(const ethcnn_lstm_samples* s) { return s ? s->skipped : ETHCNN_ERR_ARG; }

extern "C" int ethcnn_lstm_samples_build_from_records(ethcnn_lstm_samples* s, const uint8_t* records, size_t nbytes) {
    if (!s) return ETHCNN_ERR_ARG;
    if (!records && nbytes) return lerr(s, ETHCNN_ERR_ARG, "null records");
    if (int rc = begin(s)) return rc;
    if (nbytes == 0 || nbytes % kRecIn) return lerr(s, ETHCNN_ERR_FORMAT, "%zu bytes is not a whole number of %d-byte records", nbytes, kRecIn);
    const int64_t nrec = (int64_t)(nbytes / kRecIn);
    Plan pl;
    plan(nrec, [&](int64_t r) { return header_of(records + (size_t)r * kRecIn); }, &pl);
    return build(s, nullptr, records, nrec, pl);
}

extern "C" int ethcnn_lstm_samples_build_from_set(ethcnn_lstm_samples* s, ethcnn_samples* set) {
    if (!s) return ETHCNN_ERR_ARG;
    if (!set) return lerr(s, ETHCNN_ERR_ARG, "null sample set");
    if (int rc = begin(s)) return rc;
    if (set->kind != ethcnn::samples::kKindInter)
        return lerr(s, ETHCNN_ERR_FORMAT, "a set of %d-byte All-Intra records holds no residuals: ETH-LSTM samples come from an inter set", set->record_bytes());
    if (!set->built || set->count == 0 || !set->data) return lerr(s, ETHCNN_ERR_FORMAT, "the sample set is not built or holds no records");
    if (set->c != s->c) return lerr(s, ETHCNN_ERR_ARG, "the two sample sets live on different contexts");
    ethcnn_ctx* c = s->c;
    const int64_t nrec = set->count;
    // the selection: the headers leave HBM as 8 bytes a record, the host scans them (this scratch is gone before build() holds its
    // buffers against max_bytes, and is not part of that sum)
    Header* d_hdr = nullptr;
    if (hipMalloc((void**)&d_hdr, (size_t)nrec * sizeof(Header)) != hipSuccess) {
        (void)hipGetLastError();
        return lerr(s, ETHCNN_ERR_NOMEM, "%zu bytes of record headers do not fit in device memory", (size_t)nrec * sizeof(Header));
    }
    std::vector<Header> hdr((size_t)nrec);
    c->done_armed = 0;
    launch_headers(c->stream, set->data, (long)nrec, d_hdr, c->cus > 0 ? c->cus : 256);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(hdr.data(), d_hdr, (size_t)nrec * sizeof(Header), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_hdr);
    if (e != hipSuccess) return lerr(s, ETHCNN_ERR_DEVICE, "record headers: %s", hipGetErrorString(e));
    Plan pl;
    plan(nrec, [&](int64_t r) { return hdr[(size_t)r]; }, &pl);
    return build(s, set->data, nullptr, nrec, pl);
}

// ---- measurement entries (include/ethcnn.h): the kernels alone on the caller's device buffers and the float4 copy they are judged
// against, asynchronous; what scripts/lstm_samples_rate.py times
extern "C" int ethcnn_bench_lstm_repack(ethcnn_ctx* c, const uint8_t* d_records, int64_t nrecords, int64_t first, int n, int slot,
                                                 uint8_t* d_picture) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!d_records || !d_picture || ((uintptr_t)d_records | (uintptr_t)d_picture) % 16) return set_err(c, ETHCNN_ERR_ARG, "null or not 16-byte aligned buffer");
    if (slot < 0 || slot > 3) return set_err(c, ETHCNN_ERR_ARG, "QP slot %d outside 0..3", slot);
    if (first < 0 || n < 0 || first + n > nrecords) return set_err(c, ETHCNN_ERR_ARG, "records [%lld, %lld) outside 0..%lld", (long long)first, (long long)(first + n), (long long)nrecords);
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;
    launch_repack(c->stream, d_records, (long)nrecords, (long)first, n, slot, d_picture, c->cus > 0 ? c->cus : 256);
    HIPCHK(c, hipGetLastError());
    return ETHCNN_OK;
}

extern "C" int ethcnn_bench_lstm_gather(ethcnn_ctx* c, const uint8_t* d_records, int64_t nrecords, const float* d_vectors,
                                                 const int64_t* d_heads, const int64_t* d_strides, int64_t nheads, int slot, uint8_t* d_samples) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!d_records || !d_vectors || !d_heads || !d_strides || !d_samples || ((uintptr_t)d_records | (uintptr_t)d_vectors | (uintptr_t)d_samples) % 4)
        return set_err(c, ETHCNN_ERR_ARG, "null or misaligned buffer");
    if (slot < 0 || slot > 3 || nrecords < 0 || nheads < 0) return set_err(c, ETHCNN_ERR_ARG, "bad slot or count");
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;
    launch_sample_gather(c->stream, d_records, d_vectors, d_heads, d_strides, (long)nheads, slot, d_samples, c->cus > 0 ? c->cus : 256);
    HIPCHK(c, hipGetLastError());
    return ETHCNN_OK;
}

extern "C" int ethcnn_bench_copy(ethcnn_ctx* c, const void* d_src, void* d_dst, size_t nbytes) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!d_src || !d_dst || ((uintptr_t)d_src | (uintptr_t)d_dst | nbytes) % 16) return set_err(c, ETHCNN_ERR_ARG, "null buffer, or an address or size that is not a multiple of 16");
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;
    launch_copy16(c->stream, (const uint8_t*)d_src, (uint8_t*)d_dst, (long)nbytes, c->cus > 0 ? c->cus : 256);
    HIPCHK(c, hipGetLastError());
    return ETHCNN_OK;
}

extern "C" int ethcnn_lstm_samples_read(ethcnn_lstm_samples* s, int64_t first, int64_t n, uint8_t* out) {
    if (!s) return ETHCNN_ERR_ARG;
    if (!s->built) return lerr(s, ETHCNN_ERR_ARG, "the set is not built (ethcnn_lstm_samples_build_from_*)");
    if (first < 0 || n < 0 || first + n > s->count)
        return lerr(s, ETHCNN_ERR_ARG, "samples [%lld, %lld) outside 0..%lld", (long long)first, (long long)(first + n), (long long)s->count);
    if (n == 0) return ETHCNN_OK;
    if (!out) return lerr(s, ETHCNN_ERR_ARG, "null output buffer");
    ethcnn_ctx* c = s->c;
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipMemcpyAsync(out, s->data + (size_t)first * kRecOut, (size_t)n * kRecOut, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? ETHCNN_OK : lerr(s, ETHCNN_ERR_DEVICE, "read: %s", hipGetErrorString(e));
}

extern "C" int ethcnn_lstm_samples_write(ethcnn_lstm_samples* s, const char* path) {
    if (!s) return ETHCNN_ERR_ARG;
    if (!path) return lerr(s, ETHCNN_ERR_ARG, "null path");
    if (!s->built) return lerr(s, ETHCNN_ERR_ARG, "the set is not built (ethcnn_lstm_samples_build_from_*)");
    const int64_t piece = std::max<int64_t>(1, (int64_t)(kIoBytes / kRecOut));
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long)getpid());  // never a partial sample file
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f) return lerr(s, ETHCNN_ERR_IO, "cannot open %s for writing: %s", tmp.c_str(), std::strerror(errno));
    std::vector<uint8_t> buf((size_t)std::min<int64_t>(piece, std::max<int64_t>(s->count, 1)) * kRecOut);
    int rc = 0;
    for (int64_t j = 0; j < s->count && !rc; j += piece) {
        const int64_t n = std::min(piece, s->count - j);
        rc = ethcnn_lstm_samples_read(s, j, n, buf.data());
        if (!rc && std::fwrite(buf.data(), kRecOut, (size_t)n, f) != (size_t)n)
            rc = lerr(s, ETHCNN_ERR_IO, "write to %s failed: %s", tmp.c_str(), std::strerror(errno));
    }
    if (std::fclose(f) != 0 && !rc) rc = lerr(s, ETHCNN_ERR_IO, "close of %s failed", tmp.c_str());
    if (!rc && std::rename(tmp.c_str(), path) != 0) rc = lerr(s, ETHCNN_ERR_IO, "rename %s -> %s failed: %s", tmp.c_str(), path, std::strerror(errno));
    if (rc) std::remove(tmp.c_str());
    return rc;
}
