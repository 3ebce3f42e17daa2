// ethcnn_narrow.cpp -- high-bit-depth and non-4:2:0 sources (include/ethcnn.h): the source format of the file entries, the host form
// of the narrowing rule, and the device entries around k_narrow_luma (ethcnn_narrow.h).  The host entry that narrows while it fills the
// staging ring, and the file entries, live with the ring in ethcnn_host.cpp.
#include "ethcnn_ctx.h"
#include "ethcnn_narrow.h"

using namespace ethcnn::narrow;

namespace ethcnn {
namespace narrow {

void narrow_row(const uint16_t* src, uint8_t* dst, size_t n, int shift, bool nt) {
    size_t x = 0;
#if defined(__SSE2__)
    // sixteen samples per step: logical shift, min(s, 255) as s - (s -sat 255) (SSE2 has no unsigned 16-bit minimum), then the pack
    // instruction, whose signed saturation no longer has anything to do
    const __m128i vshift = _mm_cvtsi32_si128(shift), v255 = _mm_set1_epi16(255);
    if (nt)  // (streaming stores need a 16-byte aligned destination: scalar up to it)
        for (; x < n && ((uintptr_t)(dst + x) & 15) != 0; ++x) dst[x] = (uint8_t)std::min(src[x] >> shift, 255);
    for (; x + 16 <= n; x += 16) {
        __m128i a = _mm_srl_epi16(_mm_loadu_si128((const __m128i*)(src + x)), vshift);
        __m128i b = _mm_srl_epi16(_mm_loadu_si128((const __m128i*)(src + x + 8)), vshift);
        a = _mm_sub_epi16(a, _mm_subs_epu16(a, v255));
        b = _mm_sub_epi16(b, _mm_subs_epu16(b, v255));
        const __m128i r = _mm_packus_epi16(a, b);
        if (nt) _mm_stream_si128((__m128i*)(dst + x), r);
        else _mm_storeu_si128((__m128i*)(dst + x), r);
    }
#else
    (void)nt;
#endif
    for (; x < n; ++x) dst[x] = (uint8_t)std::min(src[x] >> shift, 255);
}

}  // namespace narrow
}  // namespace ethcnn

static bool format_ok(const ethcnn_source_format* f) {
    return f && f->bit_depth >= 8 && f->bit_depth <= 16 &&
           (f->chroma_format == 400 || f->chroma_format == 420 || f->chroma_format == 422 || f->chroma_format == 444);
}

extern "C" int ethcnn_narrow_rows_host(const uint16_t* src16, uint8_t* dst8, size_t n, int bit_depth) {
    if ((!src16 || !dst8) && n) return ETHCNN_ERR_ARG;
    if (bit_depth < 8 || bit_depth > 16) return ETHCNN_ERR_ARG;
    narrow_row(src16, dst8, n, bit_depth - 8, false);
    return ETHCNN_OK;
}

extern "C" int ethcnn_source_frame_bytes(const ethcnn_source_format* fmt, int w, int h, int64_t* luma_bytes, int64_t* frame_bytes) {
    if (!format_ok(fmt) || w <= 0 || h <= 0) return ETHCNN_ERR_ARG;
    const int64_t bps = fmt->bit_depth > 8 ? 2 : 1, luma = (int64_t)w * h;
    int64_t chroma = 0;
    if (fmt->chroma_format == 420) {
        // 8-bit 4:2:0 is the reference's own w * h * 3 // 2, odd sizes included (video_to_cu_depth.py:136); elsewhere two whole planes
        if (fmt->bit_depth == 8) chroma = luma * 3 / 2 - luma;
        else if (w % 2 || h % 2) return ETHCNN_ERR_ARG;
        else chroma = luma / 2;
    } else if (fmt->chroma_format == 422) {
        if (w % 2) return ETHCNN_ERR_ARG;
        chroma = luma;
    } else if (fmt->chroma_format == 444) {
        chroma = 2 * luma;
    }
    if (luma_bytes) *luma_bytes = luma * bps;
    if (frame_bytes) *frame_bytes = (luma + chroma) * bps;
    return ETHCNN_OK;
}

extern "C" int ethcnn_set_source_format(ethcnn_ctx* c, const ethcnn_source_format* fmt) {
    if (!c) return ETHCNN_ERR_ARG;
    if (!fmt) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_set_source_format: null format");
    if (!format_ok(fmt))
        return set_err(c, ETHCNN_ERR_ARG, "ethcnn_set_source_format: bit depth %d / chroma format %d (8..16; 400, 420, 422 or 444)", fmt->bit_depth,
                       fmt->chroma_format);
    c->src_fmt = *fmt;
    return ETHCNN_OK;
}

extern "C" int ethcnn_get_source_format(const ethcnn_ctx* c, ethcnn_source_format* fmt) {
    if (!c || !fmt) return ETHCNN_ERR_ARG;
    *fmt = c->src_fmt;
    return ETHCNN_OK;
}

extern "C" int ethcnn_set_narrow_chunk(ethcnn_ctx* c, int frames) {
    if (!c) return ETHCNN_ERR_ARG;
    if (frames < 0) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_set_narrow_chunk: %d frames", frames);
    c->narrow_chunk = frames;
    return ETHCNN_OK;
}

extern "C" int ethcnn_narrow_luma_device(ethcnn_ctx* c, const uint16_t* d_src16, int w, int h, ptrdiff_t pitch_bytes, ptrdiff_t fstride_bytes,
                                         int nframes, int bit_depth, uint8_t* d_dst8, ptrdiff_t dst_pitch, ptrdiff_t dst_fstride) {
    if (!c || !d_src16 || !d_dst8 || nframes < 0) return c ? set_err(c, ETHCNN_ERR_ARG, "ethcnn_narrow_luma_device: null pointer / negative frame count") : ETHCNN_ERR_ARG;
    if (w <= 0 || h <= 0) return set_err(c, ETHCNN_ERR_ARG, "bad frame size %dx%d", w, h);
    if (bit_depth < 8 || bit_depth > 16) return set_err(c, ETHCNN_ERR_ARG, "ethcnn_narrow_luma_device: bit depth %d (8..16)", bit_depth);
    if (reinterpret_cast<uintptr_t>(d_src16) % 2 || pitch_bytes % 2 || pitch_bytes < 2 * (ptrdiff_t)w)
        return set_err(c, ETHCNN_ERR_ARG, "ethcnn_narrow_luma_device: the source must be 2-byte aligned with an even pitch of at least %td bytes (pitch %td)",
                       2 * (ptrdiff_t)w, pitch_bytes);
    if (nframes > 1 && (fstride_bytes % 2 || fstride_bytes < (ptrdiff_t)(h - 1) * pitch_bytes + 2 * (ptrdiff_t)w))
        return set_err(c, ETHCNN_ERR_ARG, "ethcnn_narrow_luma_device: frame stride %td is odd or shorter than a frame", fstride_bytes);
    const int rw = roundup16(w);
    if (reinterpret_cast<uintptr_t>(d_dst8) % 16 || dst_pitch % 16 || dst_pitch < rw)
        return set_err(c, ETHCNN_ERR_ARG, "ethcnn_narrow_luma_device: the destination must be 16-byte aligned with a pitch that is a multiple of 16 and at least %d (pitch %td)",
                       rw, dst_pitch);
    if (nframes > 1 && (dst_fstride % 16 || dst_fstride < (ptrdiff_t)(h - 1) * dst_pitch + rw))
        return set_err(c, ETHCNN_ERR_ARG, "ethcnn_narrow_luma_device: destination frame stride %td is no multiple of 16 or shorter than a frame", dst_fstride);
    if ((int64_t)nframes * h * ((rw / 16 + 63) / 64) > INT32_MAX)
        return set_err(c, ETHCNN_ERR_ARG, "ethcnn_narrow_luma_device: %d frames of %d rows are more than one launch covers", nframes, h);
    if (nframes == 0) return ETHCNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    c->done_armed = 0;
    (void)hipGetLastError();
    launch_narrow(c->stream, reinterpret_cast<const uint8_t*>(d_src16), w, h, (long)pitch_bytes, (long)fstride_bytes, nframes, bit_depth - 8, d_dst8,
                  (long)dst_pitch, (long)dst_fstride, c->cus);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return set_err(c, ETHCNN_ERR_DEVICE, "launch of the narrowing kernel failed: %s", hipGetErrorString(le));
    return serial_end(c);  // (a pipelined tile stage that follows reads what this launch writes: it has to wait for the main stream)
}

// frames per chunk of ethcnn_predict_luma16_device: whole frames, the narrow buffer bounded by kDefaultChunkBytes unless a chunk is set
static int64_t narrow_chunk_frames(int64_t plane, int64_t nframes, int chunk) {
    return std::min<int64_t>(nframes, chunk > 0 ? (int64_t)chunk : std::max<int64_t>(1, kDefaultChunkBytes / plane));
}

extern "C" int ethcnn_predict_luma16_device(ethcnn_ctx* c, const uint16_t* d_luma16, int w, int h, ptrdiff_t pitch_bytes, ptrdiff_t fstride_bytes,
                                            int nframes, int bit_depth, int qp, float* d_probs) {
    if (!c || !d_luma16 || !d_probs || nframes < 0) return c ? set_err(c, ETHCNN_ERR_ARG, "null pointer / negative frame count") : ETHCNN_ERR_ARG;
    if (!c->have_weights) return set_err(c, ETHCNN_ERR_NOWEIGHTS, "no weights loaded");
    if (w <= 0 || h <= 0) return set_err(c, ETHCNN_ERR_ARG, "bad frame size %dx%d", w, h);
    if (nframes == 0) return ETHCNN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // the narrowed picture: pitch roundup16(width), its pad columns zero.  The predictor pads every picture with zeros up to whole CTUs
    // (video_to_cu_depth.py:46-59), so the padded plane of width roundup16(width) IS the same picture: it is handed on with that width,
    // which gives every narrowed picture 16-byte aligned rows (the fast CTU-load form, the single-launch small pass)
    const int rw = roundup16(w);
    const int64_t plane = (int64_t)rw * h, F = narrow_chunk_frames(plane, nframes, c->narrow_chunk);
    const size_t need = (size_t)(F * plane);
    if (need > c->narrow_cap) {  // before anything runs
        size_t free_b = 0, total_b = 0;
        HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
        if (need > free_b + c->narrow_cap)
            return set_err(c, ETHCNN_ERR_NOMEM, "ethcnn_predict_luma16_device: a chunk of %lld frames needs a narrow buffer of %zu bytes on the device; %zu are free",
                           (long long)F, need, free_b + c->narrow_cap);
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (an earlier call may still read the buffer that goes)
        if (c->narrow_buf) (void)hipFree(c->narrow_buf);
        c->narrow_buf = nullptr, c->narrow_cap = 0;
        if (hipMalloc((void**)&c->narrow_buf, need) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(c, ETHCNN_ERR_NOMEM, "ethcnn_predict_luma16_device: a narrow buffer of %zu bytes does not fit on the device", need);
        }
        c->narrow_cap = need;
    }
    const size_t per_frame = (size_t)((w + 63) / 64) * ((h + 63) / 64) * kNOut;
    for (int64_t f0 = 0; f0 < nframes; f0 += F) {
        // (chunk k + 1 overwrites the buffer that the passes of chunk k read: every pass ends on the main stream, its CTU-load stage
        // included -- the trunk waits for it --, so main-stream order is enough)
        const int nf = (int)std::min<int64_t>(F, nframes - f0);
        int rc = ethcnn_narrow_luma_device(c, reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(d_luma16) + f0 * fstride_bytes), w, h,
                                           pitch_bytes, fstride_bytes, nf, bit_depth, c->narrow_buf, rw, (ptrdiff_t)plane);
        if (rc == 0) rc = ethcnn_predict_luma_device(c, c->narrow_buf, rw, h, rw, (ptrdiff_t)plane, nf, qp, d_probs + (size_t)f0 * per_frame);
        if (rc) return rc;
    }
    return ETHCNN_OK;
}
