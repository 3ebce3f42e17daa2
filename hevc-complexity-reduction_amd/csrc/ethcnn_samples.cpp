// ethcnn_samples.cpp -- host side of the sample sets (include/ethcnn.h "sample sets"): validation and counting of the sequences, the
// build pipeline (fill threads -> page-locked staging -> HBM -> cut kernel, two chunks in flight), read-back and the file writer.
// Mirrors Extract_Data/extract_data_AI.py and extract_data_LDP_LDB_RA.py of the reference (kernels: ethcnn_samples_kernels.hip).
#include <fcntl.h>

#include "ethcnn_ctx.h"
#include "ethcnn_samples.h"

using namespace ethcnn::samples;

namespace {
constexpr size_t kChunkBytes = 48u << 20;  // staging per chunk of frames (two chunks in flight)
constexpr size_t kIoBytes = 64u << 20;     // read-back / file-writer piece

int serr(ethcnn_samples* s, int code, const char* fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    s->err = buf;
    return code;
}

size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

int check_qps(int kind, const int* qps, int nqps, std::string* why) {
    char buf[128];
    if (kind != kKindAi && kind != kKindInter) {
        std::snprintf(buf, sizeof buf, "kind must be %d (All-Intra) or %d (inter), got %d", kKindAi, kKindInter, kind);
    } else if (!qps || (kind == kKindAi ? (nqps < 1 || nqps > 52) : nqps != 4)) {
        std::snprintf(buf, sizeof buf, kind == kKindAi ? "the QP list must hold 1..52 entries, got %d" : "an inter set takes exactly four QPs, got %d", nqps);
    } else {
        for (int i = 0; i < nqps; ++i) {
            if (qps[i] < 0 || qps[i] > 51) {
                std::snprintf(buf, sizeof buf, "QP %d outside 0..51", qps[i]);
                *why = buf;
                return ETHCNN_ERR_ARG;
            }
            for (int k = 0; k < i; ++k)
                if (qps[k] == qps[i]) {
                    std::snprintf(buf, sizeof buf, "QP %d is listed twice", qps[i]);
                    *why = buf;
                    return ETHCNN_ERR_ARG;
                }
        }
        return 0;
    }
    *why = buf;
    return ETHCNN_ERR_ARG;
}

// encode_to_display_order (extract_data_LDP_LDB_RA.py:68-82): frame i of `n` in encoding order -> its place in the files
int64_t display_of(int order, int64_t i, int64_t n) {
    if (order != ETHCNN_SAMPLES_ORDER_RA || i == 0) return i;
    static const int table[8] = {7, 3, 1, 0, 2, 5, 4, 6};
    const int64_t gop = (i - 1) / 8, len = std::min<int64_t>(n - 1 - gop * 8, 8);
    int k = (int)((i - 1) % 8), at = -1;
    for (int e = 0; e < 8; ++e)  // the table without the entries a short last GOP does not have
        if (table[e] < len && k-- == 0) at = table[e];
    return 1 + at + gop * 8;
}

struct Fds {
    std::vector<int> v;
    ~Fds() {
        for (int fd : v)
            if (fd >= 0) close(fd);
    }
};

struct Staging {
    uint8_t* h[2] = {nullptr, nullptr};
    uint8_t* d[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    ~Staging() {
        for (int i = 0; i < 2; ++i) {
            if (h[i]) (void)hipHostFree(h[i]);
            if (d[i]) (void)hipFree(d[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    }
};

// geometry + alignment checks of one cut, then the launch (asynchronous on the context's stream).  bps = 2 (All-Intra only): the luma
// holds 16-bit samples, pitch and frame stride stay in bytes, and the records take min(s >> shift, 255)
int cut(ethcnn_ctx* c, std::string* why, int kind, const int* qps, int nqps, int w, int h, int nframes, const uint8_t* const* luma,
        const ptrdiff_t* pitch, const ptrdiff_t* fstride, const uint8_t* const* labels, int frame0, int seq, uint8_t* out, int bps = 1,
        int shift = 0) {
    char buf[256];
    const int nplanes = kind == kKindAi ? 1 : 4;
    auto bad = [&](const char* m) {
        *why = m;
        return ETHCNN_ERR_ARG;
    };
    if (w < 64 || h < 64 || w > 65535 || h > 65535) {
        std::snprintf(buf, sizeof buf, "bad frame size %dx%d (64..65535)", w, h);
        return bad(buf);
    }
    if (nframes < 0 || !luma || !pitch || !fstride || !labels || !out) return bad("null argument or negative frame count");
    if (frame0 < 0 || seq < 0 || seq > 65535) return bad("frame number must be >= 0 and the sequence number in 0..65535");
    if ((uintptr_t)out % (kind == kKindAi ? 16 : 4)) return bad("the record buffer must be 16-byte (inter: 4-byte) aligned");
    CutArgs a{};
    uintptr_t bits = 0, lbits = 0;
    const ptrdiff_t row_bytes = (ptrdiff_t)w * bps;
    for (int p = 0; p < nplanes; ++p) {
        if (!luma[p] || pitch[p] < row_bytes || (nframes > 1 && fstride[p] < pitch[p] * (ptrdiff_t)(h / 64 * 64 - 1) + row_bytes))
            return bad(bps == 1 ? "null plane, pitch below the width or frame stride below a frame"
                                : "null plane, pitch below 2 * width bytes or frame stride below a frame");
        if (bps == 2 && (((uintptr_t)luma[p] | (uintptr_t)pitch[p] | (uintptr_t)fstride[p]) & 1))
            return bad("16-bit luma must be 2-byte aligned, with an even pitch and an even frame stride in bytes");
        a.luma[p] = luma[p];
        a.pitch[p] = (long)pitch[p];
        a.fstride[p] = (long)fstride[p];
        bits |= (uintptr_t)luma[p] | (uintptr_t)pitch[p] | (nframes > 1 ? (uintptr_t)fstride[p] : 0);
    }
    a.lw = w / 16;
    a.label_fstride = (long)a.lw * (h / 16);
    lbits = (uintptr_t)a.lw | (nframes > 1 ? (uintptr_t)a.label_fstride : 0);
    for (int q = 0; q < nqps; ++q) {
        if (!labels[q]) return bad("null label plane");
        a.label[kind == kKindAi ? qps[q] : q] = labels[q];
        if (kind == kKindInter) a.qps[q] = qps[q];
        lbits |= (uintptr_t)labels[q];
    }
    a.label_al4 = (lbits & 3) == 0;
    a.width = w;
    a.height = h;
    a.nl = h / 64;
    a.nc = w / 64;
    a.nrec = (long)nframes * a.nl * a.nc;
    a.frame0 = frame0;
    a.seq = seq;
    a.out = out;
    a.deep = bps == 2;
    a.shift = shift;
    c->done_armed = 0;  // the context's completion word does not cover this launch
    launch_cut(c->stream, kind, a, (bits & 15) == 0 ? 16 : ((bits & 3) == 0 ? 4 : 1), c->cus > 0 ? c->cus : 256);
    if (hipGetLastError() != hipSuccess) {
        *why = "cut kernel launch failed";
        return ETHCNN_ERR_DEVICE;
    }
    return 0;
}
}  // namespace

extern "C" int ethcnn_samples_create(ethcnn_ctx* c, int kind, const int* qps, int nqps, int frame_order, uint64_t max_bytes,
                                     ethcnn_samples** out) {
    if (!out) return c ? set_err(c, ETHCNN_ERR_ARG, "null output pointer") : ETHCNN_ERR_ARG;
    *out = nullptr;
    std::string why;
    if (int rc = check_qps(kind, qps, nqps, &why)) return c ? set_err(c, rc, "%s", why.c_str()) : rc;
    if (frame_order != ETHCNN_SAMPLES_ORDER_ENCODE && !(frame_order == ETHCNN_SAMPLES_ORDER_RA && kind == kKindInter))
        return c ? set_err(c, ETHCNN_ERR_ARG, "frame order %d (0 = as stored; 1 = Random-Access table, inter sets only)", frame_order) : ETHCNN_ERR_ARG;
    ethcnn_samples* s = new (std::nothrow) ethcnn_samples;
    if (!s) return c ? set_err(c, ETHCNN_ERR_NOMEM, "out of memory") : ETHCNN_ERR_NOMEM;
    s->c = c;
    s->kind = kind;
    s->order = frame_order;
    s->nqps = nqps;
    std::memcpy(s->qps, qps, sizeof(int) * nqps);
    s->max_bytes = max_bytes;
    *out = s;
    return ETHCNN_OK;
}

extern "C" void ethcnn_samples_destroy(ethcnn_samples* s) {
    if (!s) return;
    if (s->data) {
        (void)hipSetDevice(s->c->device);
        (void)hipStreamSynchronize(s->c->stream);
        (void)hipFree(s->data);
    }
    delete s;
}

extern "C" const char* ethcnn_samples_last_error(const ethcnn_samples* s) { return s ? s->err.c_str() : "sample set is NULL"; }
extern "C" int64_t ethcnn_samples_count(const ethcnn_samples* s) { return s ? s->count : ETHCNN_ERR_ARG; }
extern "C" int ethcnn_samples_record_bytes(const ethcnn_samples* s) { return s ? s->record_bytes() : ETHCNN_ERR_ARG; }

extern "C" int ethcnn_samples_add_sequence(ethcnn_samples* s, int w, int h, const char* const* yuv_paths, int nyuv,
                                           const char* const* label_paths, int nlabels) {
    if (!s) return ETHCNN_ERR_ARG;
    if (s->built) return serr(s, ETHCNN_ERR_ARG, "the set is built: sequences are added before ethcnn_samples_build");
    const int nplanes = s->kind == kKindAi ? 1 : 4;
    if (!yuv_paths || !label_paths || nyuv != nplanes || nlabels != s->nqps)
        return serr(s, ETHCNN_ERR_ARG, "a sequence of this set takes %d YUV path(s) and %d label path(s), got %d and %d", nplanes, s->nqps, nyuv, nlabels);
    for (int i = 0; i < nyuv; ++i)
        if (!yuv_paths[i]) return serr(s, ETHCNN_ERR_ARG, "null YUV path");
    for (int i = 0; i < nlabels; ++i)
        if (!label_paths[i]) return serr(s, ETHCNN_ERR_ARG, "null label path");
    if (w < 64 || h < 64 || w % 8 || h % 8 || w > 65535 || h > 65535)  // read_info_frame asserts the multiple of 8; below 64 there is no whole CTU
        return serr(s, ETHCNN_ERR_FORMAT, "%s: frame size %dx%d: width and height must be multiples of 8, 64..65535", yuv_paths[0], w, h);
    if (s->kind == kKindInter && s->seqs.size() >= 65536) return serr(s, ETHCNN_ERR_ARG, "more than 65536 sequences (the header holds 16 bits)");
    const ethcnn_source_format fmt{s->bit_depth, s->chroma};
    const bool plain = fmt.bit_depth == 8 && fmt.chroma_format == 420;
    int64_t luma_bytes = 0, frame_bytes = 0;
    if (ethcnn_source_frame_bytes(&fmt, w, h, &luma_bytes, &frame_bytes) != ETHCNN_OK)
        return serr(s, ETHCNN_ERR_ARG, "%s: no %dx%d frame of whole planes at %d bits, chroma format %d", yuv_paths[0], w, h, fmt.bit_depth,
                    fmt.chroma_format);
    const int64_t label_bytes = (int64_t)(h / 16) * (w / 16);
    ethcnn_samples::Seq q;
    q.w = w;
    q.h = h;
    q.bit_depth = fmt.bit_depth;
    q.chroma = fmt.chroma_format;
    q.luma_bytes = luma_bytes;
    q.frame_bytes = frame_bytes;
    q.frames = -1;
    struct stat st;
    for (int i = 0; i < nyuv; ++i) {
        if (stat(yuv_paths[i], &st) != 0) return serr(s, ETHCNN_ERR_IO, "cannot stat %s: %s", yuv_paths[i], std::strerror(errno));
        if (st.st_size % frame_bytes && plain)
            return serr(s, ETHCNN_ERR_FORMAT, "%s: size %lld is not a multiple of the %dx%d 4:2:0 frame size %lld", yuv_paths[i],
                        (long long)st.st_size, w, h, (long long)frame_bytes);
        if (st.st_size % frame_bytes)
            return serr(s, ETHCNN_ERR_FORMAT, "%s: size %lld is not a multiple of the %dx%d frame size %lld at %d bits, chroma format %d (ethcnn_samples_set_source_format)",
                        yuv_paths[i], (long long)st.st_size, w, h, (long long)frame_bytes, fmt.bit_depth, fmt.chroma_format);
        const int64_t n = st.st_size / frame_bytes;
        if (q.frames >= 0 && n != q.frames)
            return serr(s, ETHCNN_ERR_FORMAT, "%s holds %lld frames, %s holds %lld", yuv_paths[i], (long long)n, yuv_paths[0], (long long)q.frames);
        q.frames = n;
        q.yuv.push_back(yuv_paths[i]);
    }
    if (q.frames > 0x7fffffff) return serr(s, ETHCNN_ERR_ARG, "%s: more than 2^31 - 1 frames", yuv_paths[0]);
    for (int i = 0; i < nlabels; ++i) {
        if (stat(label_paths[i], &st) != 0) return serr(s, ETHCNN_ERR_IO, "cannot stat %s: %s", label_paths[i], std::strerror(errno));
        if (st.st_size != q.frames * label_bytes)
            return serr(s, ETHCNN_ERR_FORMAT, "%s: size %lld, expected %lld frames x %d x %d label bytes = %lld", label_paths[i],
                        (long long)st.st_size, (long long)q.frames, h / 16, w / 16, (long long)(q.frames * label_bytes));
        q.labels.push_back(label_paths[i]);
    }
    const int64_t used = s->kind == kKindAi ? q.frames : std::max<int64_t>(q.frames - 1, 0);  // inter: the initial I-frame is skipped
    q.first_rec = s->count;
    q.nrec = used * (h / 64) * (w / 64);
    s->count += q.nrec;
    s->seqs.push_back(q);
    return ETHCNN_OK;
}

extern "C" int ethcnn_samples_set_source_format(ethcnn_samples* s, const ethcnn_source_format* fmt) {
    if (!s) return ETHCNN_ERR_ARG;
    if (!fmt) return serr(s, ETHCNN_ERR_ARG, "ethcnn_samples_set_source_format: null format");
    if (s->built) return serr(s, ETHCNN_ERR_ARG, "the set is built: the source format belongs to the sequences added before ethcnn_samples_build");
    if (ethcnn_source_frame_bytes(fmt, 2, 2, nullptr, nullptr) != ETHCNN_OK)  // (the one place that knows the formats)
        return serr(s, ETHCNN_ERR_ARG, "ethcnn_samples_set_source_format: bit depth %d / chroma format %d (8..16; 400, 420, 422 or 444)", fmt->bit_depth,
                    fmt->chroma_format);
    if (s->kind == kKindInter && (fmt->bit_depth != 8 || fmt->chroma_format != 420))
        return serr(s, ETHCNN_ERR_ARG, "an inter set reads HM's residual files, which are always 8-bit 4:2:0: source format %d bits / chroma format %d refused",
                    fmt->bit_depth, fmt->chroma_format);
    s->bit_depth = fmt->bit_depth;
    s->chroma = fmt->chroma_format;
    return ETHCNN_OK;
}

extern "C" int ethcnn_samples_cut16_device(ethcnn_ctx* c, const int* qps, int nqps, int width, int height, int nframes, const uint16_t* d_luma16,
                                           ptrdiff_t pitch_bytes, ptrdiff_t frame_stride_bytes, int bit_depth, const uint8_t* const* d_labels,
                                           uint8_t* d_records, int64_t record_offset) {
    if (!c) return ETHCNN_ERR_ARG;
    std::string why;
    int rc = check_qps(kKindAi, qps, nqps, &why);
    if (!rc && record_offset < 0) {
        rc = ETHCNN_ERR_ARG;
        why = "negative record offset";
    }
    if (!rc && (bit_depth < 8 || bit_depth > 16)) {
        rc = ETHCNN_ERR_ARG;
        why = "ethcnn_samples_cut16_device: bit depth " + std::to_string(bit_depth) + " (8..16)";
    }
    if (!rc) rc = hipSetDevice(c->device) == hipSuccess ? 0 : ETHCNN_ERR_DEVICE;
    if (!rc && d_records) d_records += (size_t)record_offset * (size_t)ethcnn::train::kRec;
    const uint8_t* luma = reinterpret_cast<const uint8_t*>(d_luma16);
    if (!rc) rc = cut(c, &why, kKindAi, qps, nqps, width, height, nframes, &luma, &pitch_bytes, &frame_stride_bytes, d_labels, 0, 0, d_records, 2, bit_depth - 8);
    return rc ? set_err(c, rc, "%s", why.c_str()) : ETHCNN_OK;
}

extern "C" int ethcnn_samples_cut_device(ethcnn_ctx* c, int kind, const int* qps, int nqps, int width, int height, int nframes,
                                         const uint8_t* const* d_luma, const ptrdiff_t* pitch, const ptrdiff_t* frame_stride,
                                         const uint8_t* const* d_labels, int frame_number, int seq_number, uint8_t* d_records,
                                         int64_t record_offset) {
    if (!c) return ETHCNN_ERR_ARG;
    std::string why;
    int rc = check_qps(kind, qps, nqps, &why);
    if (!rc && record_offset < 0) {
        rc = ETHCNN_ERR_ARG;
        why = "negative record offset";
    }
    if (!rc) rc = hipSetDevice(c->device) == hipSuccess ? 0 : ETHCNN_ERR_DEVICE;
    if (!rc && d_records)
        d_records += (size_t)record_offset * (size_t)(kind == kKindAi ? ethcnn::train::kRec : ethcnn::train::kRecLdp);
    if (!rc) rc = cut(c, &why, kind, qps, nqps, width, height, nframes, d_luma, pitch, frame_stride, d_labels, frame_number, seq_number, d_records);
    return rc ? set_err(c, rc, "%s", why.c_str()) : ETHCNN_OK;
}

extern "C" int ethcnn_samples_build(ethcnn_samples* s) {
    if (!s) return ETHCNN_ERR_ARG;
    ethcnn_ctx* c = s->c;
    if (!c) return serr(s, ETHCNN_ERR_ARG, "this set was created without a context: it validates and counts only");
    if (s->built) return serr(s, ETHCNN_ERR_ARG, "the set is already built");
    const size_t rb = (size_t)s->record_bytes();
    const unsigned long long total = (unsigned long long)s->count * rb;
    if (s->max_bytes && total > s->max_bytes)
        return serr(s, ETHCNN_ERR_NOMEM, "%lld records need %llu bytes, above the set's limit of %llu", (long long)s->count, total,
                    (unsigned long long)s->max_bytes);
    if (hipSetDevice(c->device) != hipSuccess) return serr(s, ETHCNN_ERR_DEVICE, "hipSetDevice(%d) failed", c->device);
    if (s->count == 0) {
        s->built = true;
        return ETHCNN_OK;
    }
    const int nplanes = s->kind == kKindAi ? 1 : 4;
    // frames per chunk and the staging size
    // (a luma plane counts its bytes in the file: two per sample above 8 bits -- the chunk is uploaded as it is, the kernel narrows)
    auto frame_bytes_of = [&](const ethcnn_samples::Seq& q) { return (size_t)nplanes * (size_t)q.luma_bytes + (size_t)s->nqps * (q.h / 16) * (q.w / 16); };
    auto chunk_frames = [&](const ethcnn_samples::Seq& q) { return (int)std::max<size_t>(1, std::min<size_t>((size_t)q.frames, kChunkBytes / frame_bytes_of(q))); };
    auto chunk_bytes = [&](const ethcnn_samples::Seq& q, int nf) {
        return nplanes * up256((size_t)nf * (size_t)q.luma_bytes) + s->nqps * up256((size_t)nf * (q.h / 16) * (q.w / 16));
    };
    size_t stage = 0;
    for (const auto& q : s->seqs)
        if (q.nrec) stage = std::max(stage, chunk_bytes(q, chunk_frames(q)));
    void* data = nullptr;
    if (hipMalloc(&data, (size_t)total) != hipSuccess) {
        (void)hipGetLastError();
        return serr(s, ETHCNN_ERR_NOMEM, "%lld records: %llu bytes do not fit in device memory", (long long)s->count, total);
    }
    Staging st;
    int rc = 0;
    {
        AffinityScope on_gpu_node(c->numa);  // page-locked memory is allocated where the calling thread runs
        for (int i = 0; i < 2 && !rc; ++i)
            if (hipHostMalloc((void**)&st.h[i], stage, hipHostMallocDefault) != hipSuccess || hipMalloc((void**)&st.d[i], stage) != hipSuccess ||
                hipEventCreateWithFlags(&st.ev[i], hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                rc = serr(s, ETHCNN_ERR_NOMEM, "cannot allocate two staging buffers of %zu bytes", stage);
            }
    }
    HostPool* pool = host_pool(c);
    struct Job { int fd; off_t off; size_t len; uint8_t* dst; };
    std::vector<Job> jobs;
    long chunk = 0;
    for (size_t iq = 0; iq < s->seqs.size() && !rc; ++iq) {
        const ethcnn_samples::Seq& q = s->seqs[iq];
        if (!q.nrec) continue;
        Fds fds;
        for (const auto* list : {&q.yuv, &q.labels})
            for (const std::string& p : *list) {
                fds.v.push_back(open(p.c_str(), O_RDONLY));
                if (fds.v.back() < 0 && !rc) rc = serr(s, ETHCNN_ERR_IO, "cannot open %s: %s", p.c_str(), std::strerror(errno));
            }
        if (rc) break;
        const int bps = q.bit_depth > 8 ? 2 : 1;
        const size_t plane = (size_t)q.luma_bytes, rowb = (size_t)q.w * bps, lplane = (size_t)(q.h / 16) * (q.w / 16);
        const off_t frame_bytes = (off_t)q.frame_bytes;
        const int per = (q.h / 64) * (q.w / 64), nfmax = chunk_frames(q);
        const int bands = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(q.h, 32), plane / (512u << 10)));
        const int64_t e_begin = s->kind == kKindAi ? 0 : 1;
        for (int64_t e0 = e_begin; e0 < q.frames && !rc; e0 += nfmax, ++chunk) {
            const int nf = (int)std::min<int64_t>(nfmax, q.frames - e0), b = (int)(chunk & 1);
            if (st.used[b] && hipEventSynchronize(st.ev[b]) != hipSuccess) {
                rc = serr(s, ETHCNN_ERR_DEVICE, "build: waiting for a staging buffer failed");
                break;
            }
            const size_t lreg = up256((size_t)nf * plane), qreg = up256((size_t)nf * lplane), bytes = nplanes * lreg + s->nqps * qreg;
            jobs.clear();
            for (int k = 0; k < nf; ++k) {
                const int64_t disp = display_of(s->order, e0 + k, q.frames);
                for (int p = 0; p < nplanes; ++p)  // luma only: chroma is never read
                    for (int bd = 0; bd < bands; ++bd) {
                        const int r0 = (int)((long)q.h * bd / bands), r1 = (int)((long)q.h * (bd + 1) / bands);
                        jobs.push_back({fds.v[p], (off_t)disp * frame_bytes + (off_t)(r0 * rowb), (size_t)(r1 - r0) * rowb,
                                        st.h[b] + p * lreg + (size_t)k * plane + (size_t)r0 * rowb});
                    }
                for (int l = 0; l < s->nqps; ++l)
                    jobs.push_back({fds.v[nplanes + l], (off_t)disp * (off_t)lplane, lplane, st.h[b] + nplanes * lreg + l * qreg + (size_t)k * lplane});
            }
            const std::function<int(int)> unit = [&](int u) -> int { return pinned_pread(jobs[u].fd, jobs[u].dst, jobs[u].len, jobs[u].off); };
            if (pool->run((int)jobs.size(), unit)) {
                rc = serr(s, ETHCNN_ERR_IO, "short read in the files of %s (frames %lld..%lld in encoding order)", q.yuv[0].c_str(), (long long)e0,
                          (long long)(e0 + nf - 1));
                break;
            }
            if (hipMemcpyAsync(st.d[b], st.h[b], bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
                rc = serr(s, ETHCNN_ERR_DEVICE, "build: upload of a chunk failed");
                break;
            }
            const uint8_t* luma[4];
            const uint8_t* labels[52];
            ptrdiff_t pitch[4], fstride[4];
            for (int p = 0; p < nplanes; ++p) {
                luma[p] = st.d[b] + p * lreg;
                pitch[p] = (ptrdiff_t)rowb;
                fstride[p] = (ptrdiff_t)plane;
            }
            for (int l = 0; l < s->nqps; ++l) labels[l] = st.d[b] + nplanes * lreg + l * qreg;
            std::string why;
            const int64_t rec0 = q.first_rec + (e0 - e_begin) * per;
            if (int r = cut(c, &why, s->kind, s->qps, s->nqps, q.w, q.h, nf, luma, pitch, fstride, labels, (int)e0, (int)iq, (uint8_t*)data + (size_t)rec0 * rb, bps, q.bit_depth - 8)) {
                rc = serr(s, r, "build: %s", why.c_str());
                break;
            }
            if (hipEventRecord(st.ev[b], c->stream) != hipSuccess) {
                rc = serr(s, ETHCNN_ERR_DEVICE, "build: hipEventRecord failed");
                break;
            }
            st.used[b] = true;
        }
    }
    const hipError_t e = hipStreamSynchronize(c->stream);  // (also before the staging buffers go, whatever happened)
    if (!rc && e != hipSuccess) rc = serr(s, ETHCNN_ERR_DEVICE, "build: %s", hipGetErrorString(e));
    if (rc) {
        (void)hipFree(data);
        return rc;
    }
    s->data = (uint8_t*)data;
    s->built = true;
    return ETHCNN_OK;
}

extern "C" int ethcnn_samples_read(ethcnn_samples* s, int64_t first, int64_t n, int permuted, uint64_t seed, uint8_t* out) {
    if (!s) return ETHCNN_ERR_ARG;
    if (!s->built) return serr(s, ETHCNN_ERR_ARG, "the set is not built (ethcnn_samples_build)");
    if (first < 0 || n < 0 || first + n > s->count) return serr(s, ETHCNN_ERR_ARG, "records [%lld, %lld) outside 0..%lld", (long long)first, (long long)(first + n), (long long)s->count);
    if (n == 0) return ETHCNN_OK;
    if (!out) return serr(s, ETHCNN_ERR_ARG, "null output buffer");
    ethcnn_ctx* c = s->c;
    const size_t rb = (size_t)s->record_bytes();
#define SCHK(call)                                                                                          \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess) {                                                                             \
            if (tmp) (void)hipFree(tmp);                                                                    \
            return serr(s, ETHCNN_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_));               \
        }                                                                                                   \
    } while (0)
    uint8_t* tmp = nullptr;
    SCHK(hipSetDevice(c->device));
    if (!permuted) {
        SCHK(hipMemcpyAsync(out, s->data + (size_t)first * rb, (size_t)n * rb, hipMemcpyDeviceToHost, c->stream));
        SCHK(hipStreamSynchronize(c->stream));
        return ETHCNN_OK;
    }
    const int64_t piece = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(kIoBytes / rb)));
    if (hipMalloc((void**)&tmp, (size_t)piece * rb) != hipSuccess) {
        (void)hipGetLastError();
        return serr(s, ETHCNN_ERR_NOMEM, "cannot allocate %zu bytes of device memory for the gather", (size_t)piece * rb);
    }
    c->done_armed = 0;
    for (int64_t j = 0; j < n; j += piece) {
        const int64_t m = std::min(piece, n - j);
        launch_gather(c->stream, s->kind, s->data, tmp, (long)(first + j), (long)m, (long)s->count, seed, 1, c->cus > 0 ? c->cus : 256);
        SCHK(hipGetLastError());
        SCHK(hipMemcpyAsync(out + (size_t)j * rb, tmp, (size_t)m * rb, hipMemcpyDeviceToHost, c->stream));
        SCHK(hipStreamSynchronize(c->stream));
    }
    (void)hipFree(tmp);
#undef SCHK
    return ETHCNN_OK;
}

extern "C" int ethcnn_samples_write(ethcnn_samples* s, const char* path, int permuted, uint64_t seed) {
    if (!s) return ETHCNN_ERR_ARG;
    if (!path) return serr(s, ETHCNN_ERR_ARG, "null path");
    if (!s->built) return serr(s, ETHCNN_ERR_ARG, "the set is not built (ethcnn_samples_build)");
    const size_t rb = (size_t)s->record_bytes();
    const int64_t piece = std::max<int64_t>(1, (int64_t)(kIoBytes / rb));
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long)getpid());  // never a partial sample file
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f) return serr(s, ETHCNN_ERR_IO, "cannot open %s for writing: %s", tmp.c_str(), std::strerror(errno));
    std::vector<uint8_t> buf((size_t)std::min<int64_t>(piece, std::max<int64_t>(s->count, 1)) * rb);
    int rc = 0;
    for (int64_t j = 0; j < s->count && !rc; j += piece) {
        const int64_t m = std::min(piece, s->count - j);
        rc = ethcnn_samples_read(s, j, m, permuted, seed, buf.data());
        if (!rc && std::fwrite(buf.data(), rb, (size_t)m, f) != (size_t)m) rc = serr(s, ETHCNN_ERR_IO, "write to %s failed: %s", tmp.c_str(), std::strerror(errno));
    }
    if (std::fclose(f) != 0 && !rc) rc = serr(s, ETHCNN_ERR_IO, "close of %s failed", tmp.c_str());
    if (!rc && std::rename(tmp.c_str(), path) != 0) rc = serr(s, ETHCNN_ERR_IO, "rename %s -> %s failed: %s", tmp.c_str(), path, std::strerror(errno));
    if (rc) std::remove(tmp.c_str());
    return rc;
}
