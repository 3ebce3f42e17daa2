/*
 * ethcnn.h -- C ABI of libethcnn.so: MI355X-native ETH-CNN CU-partition predictor.
 *
 * Drop-in boundary for the reference's predictor step (all paths relative to
 * /root/reference):
 *
 *   HM-16.5_Test_AI/source/App/TAppEncoder/TAppEncCfg.cpp:2317-2321
 *       system("python video_to_cu_depth.py <yuv> <w> <h> <qp>"), assert(status == 0)
 *   HM-16.5_Test_AI/bin/video_to_cu_depth.py  (driver: read YUV, tile, sub-batch, write)
 *   HM-16.5_Test_AI/bin/net_CNN.py            (ETH-CNN graph + batch gates)
 *   HM-16.5_Test_AI/source/Lib/TLibEncoder/TEncCu.cpp:237-261  (consumer of cu_depth.dat)
 *
 * The reference's boundary is a process boundary with files; there is no FFI in it.  The
 * functions below are what a binding for this path binds: one entry per reference
 * function on the path (cited per function).  Conventions: plain C types only, caller
 * owns every buffer, 0 = success, negative = error (ethcnn_last_error() has the text),
 * no exceptions cross the ABI, a context is not thread-safe (one per thread / per GPU).
 *
 * There is NO CPU fallback: every compute entry point runs hand-written HIP kernels on a
 * gfx950 device and fails with ETHCNN_ERR_DEVICE if none is usable.
 */
#ifndef ETHCNN_H
#define ETHCNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ethcnn_ctx ethcnn_ctx;

enum {
    ETHCNN_OK = 0,
    ETHCNN_ERR_ARG = -1,       /* bad argument */
    ETHCNN_ERR_IO = -2,        /* file open/read/write failed */
    ETHCNN_ERR_FORMAT = -3,    /* malformed checkpoint / Thr_info.txt / YUV size */
    ETHCNN_ERR_DEVICE = -4,    /* no usable gfx950 device or a HIP call failed */
    ETHCNN_ERR_NOWEIGHTS = -5, /* predict called before any ethcnn_load_* */
    ETHCNN_ERR_NOMEM = -6,
    ETHCNN_ERR_PLAN_REFUSED = -8, /* an opted-in 16-bit plan (ethcnn_set_fc1_plan 2 / 3) failed its load-time accuracy guard for the loaded
                                     weights; nothing was computed.  Plan 0 (and usually plan 2 when 3 was refused) still works. */
    ETHCNN_ERR_ROWS_TIMEOUT = -7 /* streamed input only (ethcnn_predict_luma_end / ethcnn_ldp_step_end): the kernels waited ~1 s for a CTU row
                                    that ethcnn_rows_ready never reported and gave up.  Nothing is wrong with the device: the same picture can
                                    be run again the plain way once its buffer is complete.  Every OTHER error of those calls is final. */
};

/* Geometry constants of the path (net_CNN.py:8-36). */
#define ETHCNN_CTU 64
#define ETHCNN_NOUT 21          /* 1 + 4 + 16 split probabilities per CTU            */
#define ETHCNN_NFEAT 2688       /* NUM_CONVLAYER_FLAT_FILTERS                        */
#define ETHCNN_NVEC 448         /* 64 + 128 + 256 (FC1 outputs; LDP VECTOR_LENGTH)   */
#define ETHCNN_SUB_BATCH 1024   /* video_to_cu_depth.py:64 sub_batch_size (gate scope)*/
#define ETHCNN_BLOB_FLOATS 1288210 /* 5,152,840-byte TF-V2 .data payload, fp32        */

typedef struct ethcnn_options {
    int device;            /* HIP device ordinal (default 0)                                 */
    int max_ctus_per_pass; /* workspace size in CTUs; 0 = default = maximum (131072: what the
                              kernels' 32-bit offsets cover; larger values are clamped). Frames
                              are never split across passes unless a single frame exceeds it. */
    int host_threads;      /* staging-fill threads of the host / file entry points; 0 = automatic:
                              ethcnn_host_thread_budget(local workers, usable CPUs)            */
    int reserved[5];
} ethcnn_options;

/* ---- lifecycle (replaces tf.Session()/Saver construction, video_to_cu_depth.py:22-29) */
int ethcnn_create(ethcnn_ctx** out, const ethcnn_options* opt /* may be NULL */);
void ethcnn_destroy(ethcnn_ctx* ctx);
const char* ethcnn_last_error(const ethcnn_ctx* ctx); /* ctx may be NULL: create() errors */
const char* ethcnn_version(void);

/* ---- weights (replaces saver.restore(sess, 'model_2000000_qpXX~YY.dat'),
 *      video_to_cu_depth.py:126-133).  The "blob" is the payload of a TF-V2
 *      .data-00000-of-00001 file: 36 fp32 tensors back to back in key order. */
int ethcnn_load_checkpoint(ethcnn_ctx* ctx, const char* prefix); /* prefix.index + prefix.data-00000-of-00001, crc32c-checked */
int ethcnn_load_blob(ethcnn_ctx* ctx, const float* blob, size_t nfloats);
int ethcnn_load_synthetic(ethcnn_ctx* ctx, uint64_t seed, double head_gain); /* trained blobs are absent from the reference */
int ethcnn_get_blob(const ethcnn_ctx* ctx, float* blob_out, size_t nfloats);
/* QP band -> checkpoint prefix (qp<25, <30, <35, else): video_to_cu_depth.py:126-133. */
int ethcnn_model_name_for_qp(int qp, char* out, size_t cap);

/* ---- thresholds (replaces net_CNN.get_thresholds('Thr_info.txt'), net_CNN.py:38-47:
 *      tokens [1] and [3] of the first line split on single spaces). */
int ethcnn_load_thresholds(ethcnn_ctx* ctx, const char* thr_info_path);
int ethcnn_parse_thresholds(const char* thr_info_path, float* thr_l1_lower, float* thr_l2_lower); /* no context / device needed */
int ethcnn_set_thresholds(ethcnn_ctx* ctx, float thr_l1_lower, float thr_l2_lower);
int ethcnn_get_thresholds(const ethcnn_ctx* ctx, float* thr_l1_lower, float* thr_l2_lower);

/* ---- prediction.  Replaces get_prob() (video_to_cu_depth.py:75-118) =
 *      get_Y_for_one_frame (:46-59) + tiling loop (:88-106) + get_y_conv_on_large_data
 *      (:61-73) + net_CNN.net (net_CNN.py:103-195).
 *      luma: 8-bit planes (16-bit planes: ethcnn_predict_luma16* below), `pitch` bytes between rows, `frame_stride` bytes between frames
 *      (w*h*3/2 when pointing into a 4:2:0 file image).  probs: float32
 *      [nframes][ceil(h/64)*ceil(w/64)][21], CTUs in raster order, row = [p64,p32[4],p16[16]]
 *      -- the cu_depth.dat layout TEncCu::compressCtu freads (TEncCu.cpp:237-261). */
int ethcnn_predict_luma_device(ethcnn_ctx* ctx, const uint8_t* d_luma, int width, int height,
                               ptrdiff_t pitch, ptrdiff_t frame_stride, int nframes, int qp,
                               float* d_probs); /* both pointers in HBM; asynchronous on the ctx stream */
int ethcnn_predict_luma(ethcnn_ctx* ctx, const uint8_t* luma, int width, int height,
                        ptrdiff_t pitch, ptrdiff_t frame_stride, int nframes, int qp,
                        float* probs); /* host pointers; synchronous */
/* ONE picture with STREAMED INPUT (the in-process encoder hook, INTEGRATION.md: TEncGOP hands over a 16-bit picture whose
 * conversion to 8 bits takes as long as the prediction -- the prediction runs under it):
 *   ethcnn_predict_luma_begin   queues the picture's pass on `luma` -- a tightly packed plane (pitch == width) in a buffer from
 *                               ethcnn_host_alloc that the caller has NOT filled yet -- and returns.  One picture of fewer than
 *                               8192 CTUs.  Until ethcnn_predict_luma_end no other call may be made on this context except
 *                               ethcnn_rows_ready.
 *   ethcnn_rows_ready           "luma rows [64 ctu_row_begin, 64 ctu_row_end) are in the buffer" (the last CTU row may be short).
 *                               (The call orders the caller's earlier stores, non-temporal ones included, before the report.)
 *                               Any thread, any order, each CTU row once; also BEFORE the begin of the same picture, but not before
 *                               the previous streamed call on this context has ended (a begin that FAILS consumes the picture: rows
 *                               reported for it are forgotten, and no further row of it may be reported).  Every CTU row
 *                               [0, ceil(height / 64)) must be reported: kernels that wait ~1 s for a row give up and the end call
 *                               fails with ETHCNN_ERR_ROWS_TIMEOUT (the GPU is not left hanging).  Shared with ethcnn_ldp_step_begin below.
 *   ethcnn_predict_luma_end     waits; probs (the pointer given to begin) are final when it returns ETHCNN_OK.
 * Results are bit-identical to ethcnn_predict_luma's. */
int ethcnn_predict_luma_begin(ethcnn_ctx* ctx, const uint8_t* luma, int width, int height, int qp, float* probs);
int ethcnn_rows_ready(ethcnn_ctx* ctx, int ctu_row_begin, int ctu_row_end);
int ethcnn_predict_luma_end(ethcnn_ctx* ctx);
/* Whole driver: all frames of the file from frame 0 (:135-140), writes `out_path`
 * (temp file + rename: never a partial cu_depth.dat).  *nframes_out may be NULL. */
int ethcnn_predict_yuv_file(ethcnn_ctx* ctx, const char* yuv_path, int width, int height, int qp,
                            const char* out_path, int64_t* nframes_out);

/* Multi-GPU sharding (no collective): one worker per GPU handles frames
 * [frame_begin, frame_end) and pwrites them at frame_begin * nctu * 84 into `out_path`,
 * which must already exist with its final size (frames * nctu * 84 bytes). */
int ethcnn_predict_yuv_shard(ethcnn_ctx* ctx, const char* yuv_path, int width, int height, int qp,
                             const char* out_path, int64_t frame_begin, int64_t frame_end);

/* The whole file over several GPUs from ONE process, a worker thread per listed device (thread-per-GPU form of the same split: the
 * reference's caller blocks in system(), TAppEncCfg.cpp:2317-2321, so what counts is the command's wall time -- N interpreters, N
 * checkpoint parses and N cold contexts cost more than 1/N of a short job saves).  `ctx` is worker 0 and must live on devices[0]; a
 * device may be listed more than once (several workers sharing one GPU: tests, and profiles/r06_cold_start.txt).  Workers 1.. are
 * contexts the library creates once and keeps with `ctx` (a copy of its weights, thresholds, plan; host threads: the node budget divided
 * by the worker count).  Frames [total k / n, total (k + 1) / n) to worker k, each pwriting at its offset into a temp file; one
 * rename.  Output byte-identical to ethcnn_predict_yuv_file.  ndevices == 1 is that call. */
int ethcnn_predict_yuv_file_sharded(ethcnn_ctx* ctx, const int* devices, int ndevices, const char* yuv_path, int width, int height, int qp,
                                    const char* out_path, int64_t* nframes_out);
/* the split both sharded forms use: worker k of n gets frames [floor(k F / n), floor((k + 1) F / n)).  Pure (no context, no device). */
int ethcnn_shard_range(int64_t nframes, int workers, int k, int64_t* frame_begin, int64_t* frame_end);

/* get_prob(yuv_name, ..., n_frames_start, n_frames_end, ...) (video_to_cu_depth.py:75-118): frames [frame_begin, frame_end) of the
 * file (the reference reads and discards the first n_frames_start frames, :86-87) -> an `out_path` that holds exactly those
 * frames, written to a temp file and renamed.  The reference's own call passes 0 and the frame count = ethcnn_predict_yuv_file. */
int ethcnn_predict_yuv_range(ethcnn_ctx* ctx, const char* yuv_path, int width, int height, int qp,
                             const char* out_path, int64_t frame_begin, int64_t frame_end);

/* ---- high-bit-depth and non-4:2:0 sources.  HM reads InputBitDepth 8..16 and InputChromaFormat 400 / 420 / 422 / 444 (Main10 material:
 *      UHD content, the 10-bit class-A sequences); the network was trained on 8-bit luma.
 *   THE NARROWING RULE: a deep sample is an unsigned 16-bit little-endian value s, and the picture the network sees is
 *        min(s >> (bit_depth - 8), 255),   bit_depth 8..16
 *      (depth 8: 8-bit data in 16-bit containers).  For every value a plane can hold at its depth, 0 .. 2^bit_depth - 1, this is what
 *      the in-process encoder hook computes for HM's Pel planes (tools/hm_inprocess_hook.c, convert_row); larger values clamp to 255.
 *      The host and the device implementation agree on all 65536 values at every depth.  Big-endian or MSB-aligned containers are
 *      not handled.
 *   ethcnn_narrow_rows_host      the rule over n samples on the host (SSE2, scalar elsewhere); pure: no context, no device
 *   ethcnn_narrow_luma_device    the rule over nframes planes resident in HBM, one kernel, asynchronous on the context's stream.  Source:
 *                                any 2-byte aligned address, pitch_bytes even and >= 2 width, frame_stride_bytes even.  Destination:
 *                                16-byte aligned, dst_pitch a multiple of 16 and >= roundup16(width) = (width + 15) / 16 * 16,
 *                                dst_frame_stride a multiple of 16.  Bytes [width, roundup16(width)) of every destination row are
 *                                written as zero; nothing else outside [0, width) is written, and no source sample outside a row's
 *                                width is read beyond the 16-byte line its first sample lies in.
 *   ethcnn_predict_luma16_device ethcnn_predict_luma_device for 16-bit planes in HBM: they are narrowed into a buffer the context owns
 *                                (pitch roundup16(width), pad columns zero: the predictor pads pictures with zeros up to whole CTUs, so
 *                                that plane is the same picture, with 16-byte aligned rows) and predicted from there; bit-identical to
 *                                ethcnn_predict_luma_device on the planes narrowed by the rule.  Long inputs go in chunks of whole frames:
 *                                the buffer holds at most 256 MB (or ethcnn_set_narrow_chunk frames; 0 = that default; results do not
 *                                depend on it).  A buffer that cannot be had fails with ETHCNN_ERR_NOMEM and its size in the message,
 *                                before anything runs.  Asynchronous.
 *   ethcnn_predict_luma16        the same from host pointers, synchronous: the context's fill threads narrow on the CPU while they fill
 *                                the staging ring, so one byte per sample crosses PCIe (the bus bounds the host and file entries).
 *   Source format of the FILE entries (ethcnn_predict_yuv_file, _shard, _file_sharded, _range; sharded workers inherit it):
 *      ethcnn_set_source_format / ethcnn_get_source_format; default {8, 420}, the reference's only format.  bit_depth > 8: the file
 *      holds 16-bit samples; bit_depth == 8: one byte per sample.  Planar, luma first; only luma is read.  A file whose size is not a
 *      multiple of the frame size fails with ETHCNN_ERR_FORMAT, the message names the format in force.  The Low-Delay-P entries
 *      (ethcnn_ldp_*) are NOT affected: HM's residual writer always emits 8-bit 4:2:0.
 *   Sample sets ("sample sets" below) read the same formats for All-Intra sequences: ethcnn_samples_set_source_format per set, and
 *      ethcnn_samples_cut16_device, the cut kernel over 16-bit planes in HBM.  Their records hold the picture narrowed by the rule, so a
 *      model is trained on what the predictor entries above will show it.  Inter sets keep 8-bit 4:2:0, for the reason just given.
 *   ethcnn_source_frame_bytes    pure: bytes of the luma plane and of a whole frame.  Chroma share in samples: 0 (400), w h / 2 (420),
 *                                w h (422), 2 w h (444).  8-bit 4:2:0 is exactly the reference's w * h * 3 / 2 (integer division, odd
 *                                sizes included: video_to_cu_depth.py:136); 4:2:0 at other depths needs even w and h, 4:2:2 an even w,
 *                                else ETHCNN_ERR_ARG. */
typedef struct ethcnn_source_format {
    int bit_depth;     /* 8..16 */
    int chroma_format; /* 400, 420, 422 or 444 */
} ethcnn_source_format;
int ethcnn_narrow_rows_host(const uint16_t* src16, uint8_t* dst8, size_t n, int bit_depth);
int ethcnn_narrow_luma_device(ethcnn_ctx* ctx, const uint16_t* d_src16, int width, int height, ptrdiff_t pitch_bytes,
                              ptrdiff_t frame_stride_bytes, int nframes, int bit_depth, uint8_t* d_dst8, ptrdiff_t dst_pitch,
                              ptrdiff_t dst_frame_stride);
int ethcnn_predict_luma16_device(ethcnn_ctx* ctx, const uint16_t* d_luma16, int width, int height, ptrdiff_t pitch_bytes,
                                 ptrdiff_t frame_stride_bytes, int nframes, int bit_depth, int qp, float* d_probs);
int ethcnn_predict_luma16(ethcnn_ctx* ctx, const uint16_t* luma16, int width, int height, ptrdiff_t pitch_bytes,
                          ptrdiff_t frame_stride_bytes, int nframes, int bit_depth, int qp, float* probs);
int ethcnn_set_narrow_chunk(ethcnn_ctx* ctx, int frames);
int ethcnn_set_source_format(ethcnn_ctx* ctx, const ethcnn_source_format* fmt);
int ethcnn_get_source_format(const ethcnn_ctx* ctx, ethcnn_source_format* fmt);
int ethcnn_source_frame_bytes(const ethcnn_source_format* fmt, int width, int height, int64_t* luma_bytes, int64_t* frame_bytes);

/* ---- config #5 front-end: resi_cnn (HM-16.5_Test_LDP/bin/net_CNN_LSTM_one_step.py:151-199)
 *      fed as in resi_to_cu_depth_LDP.py:72-101.  One frame; vec = float32 [nctu][448].
 *      Alignment of the device pointers: d_luma none (any byte address and pitch give the same vectors; rows that are 16-byte aligned
 *      -- address, width and pitch -- take the wide loads); d_vec 4 bytes (stored dword by dword, exactly nctu x 448 floats), else
 *      ETHCNN_ERR_ARG before anything is enqueued. */
int ethcnn_resi_vectors_device(ethcnn_ctx* ctx, const uint8_t* d_luma, int width, int height,
                               ptrdiff_t pitch, float* d_vec);
int ethcnn_resi_vectors(ethcnn_ctx* ctx, const uint8_t* luma, int width, int height,
                        ptrdiff_t pitch, float* vec);

/* ---- config #5 back-end ("next" row 1): one ETH-LSTM step + heads + gates per frame =
 *      what predict_cu_depth() fetches from sess.run (HM-16.5_Test_LDP/bin/
 *      resi_to_cu_depth_LDP.py:108-129; graph: net_CNN_LSTM_one_step.py:201-323).
 *      CNN weights: ethcnn_load_checkpoint("model_LDP_2000000_qp22~37.dat") (same 36-tensor
 *      table; only conv + FC1 are used).  LSTM weights: the 18-tensor bundle
 *      model_LDP_200000_qp{22,27,32,37}.dat, reloaded when the QP band changes (:166-179).
 *      state: float32 [nctu][2][448] = (c, h) per CTU, the layout of state.dat (:103-106,131-137);
 *      state_in NULL = zeros (i_frame <= 1).  efs = [qp/51*0.18, onehot4(i_frame % 4)].
 *      Gates are per 1024-CTU mini-batch of the frame (:118).
 *      ethcnn_lstm_step_device: device pointers to exactly nctu rows each (the kernels work in groups of 16 CTUs, and keep the
 *      surplus lanes of the last group off the caller's memory).  Alignment: d_vec, d_state_in (when given) and d_state_out 16 bytes
 *      (read as float4 / dwordx4), d_probs 4 bytes (stored dword by dword).  A pointer below its alignment is refused with
 *      ETHCNN_ERR_ARG before anything is allocated or enqueued; the text names the argument. */
#define ETHCNN_LSTM_BLOB_FLOATS 760078 /* 3,040,312-byte TF-V2 .data payload, fp32 */
int ethcnn_load_lstm_checkpoint(ethcnn_ctx* ctx, const char* prefix);
int ethcnn_load_lstm_blob(ethcnn_ctx* ctx, const float* blob, size_t nfloats);
int ethcnn_load_lstm_synthetic(ethcnn_ctx* ctx, uint64_t seed, double head_gain);
int ethcnn_get_lstm_blob(const ethcnn_ctx* ctx, float* blob_out, size_t nfloats);
int ethcnn_lstm_model_name_for_qp(int qp, char* out, size_t cap);
int ethcnn_lstm_step_device(ethcnn_ctx* ctx, const float* d_vec, const float* d_state_in /* may be NULL */,
                            int nctu, int qp, int i_frame, float* d_state_out, float* d_probs);
int ethcnn_ldp_predict_frame(ethcnn_ctx* ctx, const uint8_t* luma, int width, int height, ptrdiff_t pitch,
                             int qp, int i_frame, const float* state_in /* may be NULL */, float* state_out,
                             float* probs); /* host pointers; synchronous */
/* The same per-frame call with the recurrent (c, h) state RESIDENT in HBM between frames (the daemon's fast path:
 * state.dat is part of the reference's file protocol, but only the daemon itself ever reads it back --
 * resi_to_cu_depth_LDP.py:103-106 -- so the 2 x nctu x 3.5 KB PCIe round trip per frame is not needed):
 *   state_in != NULL          use (and upload) this state, as ethcnn_ldp_predict_frame does;
 *   state_in == NULL, i_frame <= 1   zeros (:109-110);
 *   state_in == NULL, i_frame > 1    the state the previous ethcnn_ldp_step left in HBM (error if there is none or the
 *                                     CTU count changed).
 * probs returns synchronously; ethcnn_ldp_get_state copies the new state out afterwards (off the encoder's critical
 * path: the daemon signals pred_end.sig first, then refreshes state.dat). */
int ethcnn_ldp_step(ethcnn_ctx* ctx, const uint8_t* luma, int width, int height, ptrdiff_t pitch, int qp, int i_frame,
                    const float* state_in /* may be NULL */, float* probs);
int ethcnn_ldp_get_state(ethcnn_ctx* ctx, float* state_out, size_t nfloats /* nctu * 896 */);
/* ethcnn_ldp_step with STREAMED INPUT: the frame's kernels are queued BEFORE its luma is in memory, and consume it CTU row by CTU row
 * while the caller is still filling the buffer -- the daemon's threads copying resi.yuv out of the page cache
 * (resi_to_cu_depth_LDP.py:116-118 reads the file, THEN predicts: 52 us + 115 us at 1920x1080; streamed, the transfer over PCIe
 * and the launch overheads run under the read).
 *   ethcnn_ldp_step_begin   arguments as ethcnn_ldp_step; luma MUST lie in a buffer from ethcnn_host_alloc (read in place).  Returns
 *                           once everything is queued.  Until ethcnn_ldp_step_end no other call may be made on this context
 *                           except ethcnn_rows_ready.
 *   ethcnn_rows_ready   "luma rows [64 ctu_row_begin, 64 ctu_row_end) are in the buffer" (the last CTU row may be short).  Any
 *                           thread, any order, each CTU row once; may be called BEFORE ethcnn_ldp_step_begin of the same frame, but
 *                           not before the previous streamed step has ended.  Every CTU row [0, ceil(height / 64)) must be
 *                           reported: kernels that wait ~1 s for a row give up, and ethcnn_ldp_step_end then fails with
 *                           ETHCNN_ERR_ROWS_TIMEOUT (the GPU is not left hanging; the step's INPUT state stays resident -- the state the
 *                           previous step left, or the copy of state_in --, so the frame can be run again with ethcnn_ldp_step and the
 *                           same arguments once its buffer is complete).
 *   ethcnn_ldp_step_end     waits; probs (the pointer given to begin) and the resident state are final when it returns ETHCNN_OK.
 * Results are bit-identical to ethcnn_ldp_step's. */
int ethcnn_ldp_step_begin(ethcnn_ctx* ctx, const uint8_t* luma, int width, int height, ptrdiff_t pitch, int qp, int i_frame,
                          const float* state_in /* may be NULL */, float* probs);
/* (ethcnn_rows_ready: declared with ethcnn_predict_luma_begin above) */
int ethcnn_ldp_step_end(ethcnn_ctx* ctx);
/* ---- config #5 offline: a whole residual sequence.  The result EQUALS nframes successive ethcnn_ldp_step calls on the same context, frame t
 *      carrying i_frame = i_frame_first + t, bit for bit (gates and their zero patterns included): probs[t] is that step's probs, the
 *      state left resident is the last step's (ethcnn_ldp_get_state returns it; a following ethcnn_ldp_step with state_in == NULL and
 *      the next i_frame continues from it: a daemon can be warm-started).  Input state of frame t: zeros when its i_frame <= 1, else
 *      the previous frame's output; for t == 0 with i_frame > 1: state_in when given, else the resident state (the error of
 *      ethcnn_ldp_step if there is none or it belongs to another CTU count).  efs per frame as in ethcnn_ldp_step; gates per 1024-CTU
 *      mini-batch of each frame with the context's thresholds; the weights are the ones loaded (the LSTM bundle of the QP band is the
 *      caller's choice).  i_frame_first >= 0.  What differs is the schedule: the front-end of a CHUNK of frames runs in the big
 *      multi-launch passes, the recurrence of a chunk is one launch whose blocks own their CTUs for all frames and keep (c, h) on
 *      chip, a small post-pass applies the gates.  Results do not depend on the chunk size.
 *   ethcnn_ldp_sequence_device   device pointers, asynchronous on the context's stream; d_probs float32 [nframes][nctu][21]
 *                                Row y of frame t starts at d_luma + t frame_stride + y pitch; nothing outside the width x height
 *                                pixels of a frame is read, d_state_in is read as exactly nctu rows, and nothing outside
 *                                [nframes][nctu][21] is written.  Alignment: d_luma, pitch and frame_stride none (16-byte aligned
 *                                rows take the wide loads, the result is the same); d_state_in 16 bytes when given (read as float4);
 *                                d_probs 4 bytes (touched dword by dword).  A pointer below its alignment is refused with
 *                                ETHCNN_ERR_ARG before anything is allocated or enqueued, the resident state left as it was; the
 *                                text names the argument.  frame_stride is the caller's to get right (not checked here).
 *   ethcnn_ldp_sequence          host pointers (pageable or from ethcnn_host_alloc), synchronous
 *   ethcnn_ldp_predict_yuv_file  a 4:2:0 file of residual frames (HM-16.5_Resi_Pre's resi_XX.yuv): frame k of the file is POC k, so
 *                                i_frame = k; frames [frame_begin, frame_end) are processed and out_path holds exactly those as
 *                                float32 [frames][nctu][21] (temp file + rename).  frame_begin == 0 is refused: POC 0 is the intra
 *                                picture and has no residual.  frame_begin > 1 continues from the resident state.  Only luma is read.
 *   ethcnn_ldp_set_sequence_chunk   frames per chunk; 0 = default (256 MB of vectors)
 *   ethcnn_ldp_sequence_bytes    host only, no context: the device bytes a call holds for that chunk size, F = min(nframes, chunk or
 *                                default) frames: F nctu 448 x 4 (vectors) + F nctu 21 x 4 (probabilities of the host / file entries)
 *                                + 2 x roundup16(nctu) x 896 x 4 (the two state buffers); negative for bad arguments.  A call that
 *                                cannot get its buffers fails with ETHCNN_ERR_NOMEM and this sum in the message, nothing allocated. */
int ethcnn_ldp_sequence_device(ethcnn_ctx* ctx, const uint8_t* d_luma, int width, int height, ptrdiff_t pitch, ptrdiff_t frame_stride,
                               int nframes, int qp, int i_frame_first, const float* d_state_in /* may be NULL */, float* d_probs);
int ethcnn_ldp_sequence(ethcnn_ctx* ctx, const uint8_t* luma, int width, int height, ptrdiff_t pitch, ptrdiff_t frame_stride, int nframes,
                        int qp, int i_frame_first, const float* state_in /* may be NULL */, float* probs);
int ethcnn_ldp_predict_yuv_file(ethcnn_ctx* ctx, const char* resi_yuv_path, int width, int height, int qp, const char* out_path,
                                int64_t frame_begin, int64_t frame_end);
int ethcnn_ldp_set_sequence_chunk(ethcnn_ctx* ctx, int frames);
int64_t ethcnn_ldp_sequence_bytes(int width, int height, int nframes, int chunk_frames);
/* ---- config #5 offline, group form: K = 1..8 residual sequences of ONE geometry, length and first frame number through the chain together.
 *      HM-16.5_Resi_Pre writes one resi_XX.yuv per QP of a sequence and every record of an inter sample file carries four QP slots: the
 *      members of a group are such sequences, each with its own ETH-LSTM bundle, QP, state and output.
 *      DEFINITION: for every member m, d_probs[m] and m's resident state EQUAL what ethcnn_ldp_sequence_device gives on a context that
 *      holds m's bundle and whose thresholds are m's RESOLVED pair, for d_luma[m], qp[m] and the same remaining arguments (d_state_in[m]
 *      for d_state_in), bit for bit, gates and their zero patterns included.  Member m's resolved pair is its own when
 *      ethcnn_ldp_set_thresholds_group gave it one, else the context's pair as it stands when the call is made.  The residual CNN and
 *      the stream are the context's; the context's own LSTM bundle, resident LDP state and sequence buffers are neither used nor changed.
 *      What differs is the schedule: the front-end runs per member and chunk as in the solo call; the recurrence of a run of frames is
 *      ONE launch for all members (level-major block order: every member's long chains first), the gates of a chunk ONE launch.
 *      Geometry, nframes and i_frame_first are common, so all members split into runs at the same frames (i_frame <= 1).
 *   ethcnn_ldp_group_create       k members on ctx (ETHCNN_ERR_ARG outside 1..8; text: ethcnn_last_error of the context).  Destroy the
 *                                 group before its context.  Errors of every other entry: ethcnn_ldp_group_last_error.
 *   ethcnn_ldp_group_load_lstm_checkpoint / _load_lstm_blob / _load_lstm_synthetic   member m's bundle, as the context's loaders take
 *                                 theirs (a blob holds exactly the floats of ethcnn_get_lstm_blob, else ETHCNN_ERR_ARG and the member
 *                                 keeps what it had).  Each member keeps its own device image, payload + packed kernels (6.05 MB),
 *                                 from load time on.  ethcnn_ldp_group_get_lstm_blob returns the payload.
 *   ethcnn_ldp_group_sequence_device   d_luma, qp, d_probs: arrays of k entries; d_state_in: NULL, or an array of k entries of which
 *                                 any may be NULL.  Device pointers, asynchronous on the context's stream.  Each member has ONE resident
 *                                 state buffer, owned by the group and advanced in place; input state of member m's frame 0 when
 *                                 i_frame_first > 1: d_state_in[m] when given, else m's resident state (the error of ethcnn_ldp_step,
 *                                 ETHCNN_ERR_ARG, if it is empty or belongs to another CTU count).  No member's d_probs or d_state_in
 *                                 may overlap another's d_probs.  Refused before anything is allocated or enqueued, states left as
 *                                 they were: an open streamed call (ETHCNN_ERR_ARG), no CNN weights, a member without a bundle
 *                                 (ETHCNN_ERR_NOWEIGHTS, the text names the member), a null pointer, bad geometry, nframes <= 0,
 *                                 i_frame_first < 0, a d_state_in[m] that is not 16-byte aligned or a d_probs[m] that is not 4-byte
 *                                 aligned (ETHCNN_ERR_ARG, the text names argument and member; d_luma[m], pitch and frame_stride need
 *                                 no alignment, as in the solo call).  A failure after that point drops every member's resident state.
 *                                 Buffers that lie back to back (member m + 1's at the end of member m's) do not overlap.
 *   ethcnn_ldp_group_get_state    member m's resident state, float32 [nctu][2][448]; synchronous
 *   ethcnn_ldp_group_state_ctus   the CTU count of member m's resident state; 0: none; negative: bad arguments
 *   ethcnn_ldp_group_set_chunk    frames per chunk; 0 = default (256 MB of vectors for the whole group).  Results do not depend on it.
 *   ethcnn_ldp_set_thresholds_group / ethcnn_ldp_clear_thresholds_group / ethcnn_ldp_get_thresholds_group   member m's gate pair, as ethcnn_ldp_set_thresholds_batch
 *                                 takes sequence index j's.
 *   ethcnn_ldp_group_bytes        host only, no context: the device bytes a call holds, F = min(nframes, chunk or default) frames:
 *                                 k F nctu 448 x 4 (vectors) + k x roundup16(nctu) x 896 x 4 (the resident states); negative for bad
 *                                 arguments.  Beside it, from load time: k bundle images.  A call that cannot get its buffers fails
 *                                 with ETHCNN_ERR_NOMEM and this sum in the message, before anything is allocated or enqueued. */
typedef struct ethcnn_ldp_group ethcnn_ldp_group;
int ethcnn_ldp_group_create(ethcnn_ctx* ctx, int k, ethcnn_ldp_group** out);
void ethcnn_ldp_group_destroy(ethcnn_ldp_group* grp);
const char* ethcnn_ldp_group_last_error(const ethcnn_ldp_group* grp);
int ethcnn_ldp_group_count(const ethcnn_ldp_group* grp);
int ethcnn_ldp_group_load_lstm_checkpoint(ethcnn_ldp_group* grp, int m, const char* prefix);
int ethcnn_ldp_group_load_lstm_blob(ethcnn_ldp_group* grp, int m, const float* blob, size_t nfloats);
int ethcnn_ldp_group_load_lstm_synthetic(ethcnn_ldp_group* grp, int m, uint64_t seed, double head_gain);
int ethcnn_ldp_group_get_lstm_blob(ethcnn_ldp_group* grp, int m, float* out, size_t nfloats);
int ethcnn_ldp_group_sequence_device(ethcnn_ldp_group* grp, const uint8_t* const* d_luma, int width, int height, ptrdiff_t pitch,
                                     ptrdiff_t frame_stride, int nframes, const int* qp, int i_frame_first,
                                     const float* const* d_state_in /* NULL, or entries NULL */, float* const* d_probs);
int ethcnn_ldp_group_get_state(ethcnn_ldp_group* grp, int m, float* state_out, size_t nfloats /* nctu * 896 */);
int64_t ethcnn_ldp_group_state_ctus(ethcnn_ldp_group* grp, int m);
int ethcnn_ldp_group_set_chunk(ethcnn_ldp_group* grp, int frames);
int64_t ethcnn_ldp_group_bytes(int width, int height, int nframes, int chunk_frames, int k);
int ethcnn_ldp_set_thresholds_group(ethcnn_ldp_group* grp, int m, float thr_l1_lower, float thr_l2_lower);
int ethcnn_ldp_clear_thresholds_group(ethcnn_ldp_group* grp, int m);
int ethcnn_ldp_get_thresholds_group(ethcnn_ldp_group* grp, int m, float* thr_l1_lower, float* thr_l2_lower, int* own);
/* ---- config #5 offline, batch form: up to 32 residual sequences of DIFFERENT geometry, length and first frame number through the chain
 *      together (an evaluation set, or the runs of an inter sample file), on one GPU.  The object holds up to 8 ETH-LSTM bundles; every
 *      sequence names its bundle by index, so several sequences of one QP band share one device image.
 *      DEFINITION: for every j, seqs[j].d_probs and the resident state left for sequence index j EQUAL what ethcnn_ldp_sequence_device
 *      gives with the same remaining arguments on a context that holds bundle seqs[j].bundle and whose thresholds are j's RESOLVED pair,
 *      bit for bit, gates and their zero patterns (per frame and 1024-CTU mini-batch of that sequence's own picture) included.  Index
 *      j's resolved pair is its own when ethcnn_ldp_set_thresholds_batch gave it one, else the context's pair as it stands when the call
 *      is made; no sequence's result depends on another's pair.  The residual CNN and the stream are the context's; the context's own
 *      LSTM bundle, resident LDP state and sequence buffers are neither used nor changed.
 *      What differs is the schedule: a call is cut into chunks of Fc frames common to all sequences; chunk t holds frames
 *      [t Fc, min((t + 1) Fc, nframes_j)) of every sequence that still has frames.  Per chunk the front-end runs per sequence as in the
 *      solo call, then ONE recurrence launch and ONE gate launch serve all sequences of the chunk (level-major block order; inside a
 *      level the sequences with most frames in the launch first).  A launch lasts as long as its longest member.
 *   ethcnn_ldp_batch_create       nbundles bundle places on ctx (ETHCNN_ERR_ARG outside 1..8; text: ethcnn_last_error of the context).
 *                                 Destroy the batch before its context.  Errors of every other entry: ethcnn_ldp_batch_last_error.
 *   ethcnn_ldp_batch_load_lstm_checkpoint / _load_lstm_blob / _load_lstm_synthetic / _get_lstm_blob   bundle i, as the group's take member m's
 *   ethcnn_ldp_batch_run_device   nseqs = 1..32 sequences.  Device pointers, asynchronous on the context's stream.  i_frame_first >= 1 per
 *                                 sequence (0, the intra picture, is ETHCNN_ERR_ARG here; the solo and group calls keep accepting it).
 *                                 With i_frame_first == 1 the start state is zero; above 1 it is d_state_in when given, else the resident
 *                                 state of index j (the error of ethcnn_ldp_step, ETHCNN_ERR_ARG, if that is empty or belongs to another
 *                                 CTU count).  Inside a sequence the state is always carried.  Each sequence index has ONE resident state
 *                                 buffer of its own roundup16(nctu) CTUs, owned by the batch and advanced in place.  Refused before anything
 *                                 is allocated or enqueued, every state left as it was: an open streamed call, no CNN weights, a bundle
 *                                 index that is out of range or empty (ETHCNN_ERR_NOWEIGHTS, the text names sequence and bundle), a null
 *                                 pointer, bad geometry, nframes <= 0, nseqs outside 1..32, a d_probs that overlaps another sequence's
 *                                 d_probs or d_state_in (buffers that lie back to back do not overlap), a d_state_in that is not 16-byte
 *                                 aligned or a d_probs that is not 4-byte aligned (ETHCNN_ERR_ARG, the text names argument and sequence;
 *                                 d_luma, pitch and frame_stride need no alignment).  NOT checked, the caller's to keep apart: a d_probs against
 *                                 the same sequence's d_state_in and against any d_luma.  A failure after that point drops every
 *                                 resident state.
 *   ethcnn_ldp_batch_get_state    the resident state of sequence index j, float32 [nctu][2][448]; synchronous
 *   ethcnn_ldp_batch_state_ctus   its CTU count; 0: none; negative: bad arguments
 *   ethcnn_ldp_batch_set_chunk    Fc; 0 = default: max(1, floor(256 MB / sum_j nctu_j x 1792)).  Results do not depend on it.
 *   ethcnn_ldp_set_thresholds_batch   (the gate entries of a batch and of a group carry the form LAST in their names: the families
 *                                 ethcnn_ldp_batch_* and ethcnn_ldp_group_* are closed lists, held to their members by the tests of the
 *                                 changes that made them.)  Gives sequence index j = 0..31 a gate pair of its own (thr_l1_lower, thr_l2_lower as
 *                                 ethcnn_set_thresholds takes them: it refuses no float, so neither does this).  The pair is sticky across
 *                                 calls, like the index's resident state.  ethcnn_ldp_clear_thresholds_batch: the index inherits the context's pair again.
 *                                 ethcnn_ldp_get_thresholds_batch: the resolved pair and *own = 1 (its own) or 0 (the context's, as it stands now); every
 *                                 output pointer is needed.  Host-only bookkeeping: nothing is enqueued and nothing waits.  ETHCNN_ERR_ARG:
 *                                 an index out of range, a null output pointer, an open streamed call.
 *   ethcnn_ldp_batch_bytes        host only, no context: sum_j min(nframes_j, Fc) nctu_j 1792 (vectors) + sum_j roundup16(nctu_j) 3584 (the
 *                                 resident states); negative for bad arguments.  Beside it, from load time: the bundle images.  A call that
 *                                 cannot get its buffers fails with ETHCNN_ERR_NOMEM and this sum in the message, before anything is
 *                                 allocated or enqueued.
 *   ethcnn_ldp_batch_plan         host only: for CTU counts and frame counts, Fc, the number of chunks, and per chunk four ints
 *                                 {sequences that take part, recurrence blocks at level 16, 32, 64} (sequence j: G_j, ceil(G_j / 2),
 *                                 ceil(G_j / 4) with G_j = ceil(nctu_j / 16)); at most max_chunks rows are written. */
typedef struct ethcnn_ldp_batch ethcnn_ldp_batch;
typedef struct ethcnn_ldp_batch_seq {
    const uint8_t* d_luma;
    int width, height;
    ptrdiff_t pitch, frame_stride;
    int nframes, qp, i_frame_first, bundle;
    const float* d_state_in; /* may be NULL */
    float* d_probs;          /* [nframes][nctu][21] */
} ethcnn_ldp_batch_seq;
int ethcnn_ldp_batch_create(ethcnn_ctx* ctx, int nbundles, ethcnn_ldp_batch** out);
void ethcnn_ldp_batch_destroy(ethcnn_ldp_batch* b);
const char* ethcnn_ldp_batch_last_error(const ethcnn_ldp_batch* b);
int ethcnn_ldp_batch_bundles(const ethcnn_ldp_batch* b);
int ethcnn_ldp_batch_load_lstm_checkpoint(ethcnn_ldp_batch* b, int bundle, const char* prefix);
int ethcnn_ldp_batch_load_lstm_blob(ethcnn_ldp_batch* b, int bundle, const float* blob, size_t nfloats);
int ethcnn_ldp_batch_load_lstm_synthetic(ethcnn_ldp_batch* b, int bundle, uint64_t seed, double head_gain);
int ethcnn_ldp_batch_get_lstm_blob(ethcnn_ldp_batch* b, int bundle, float* out, size_t nfloats);
int ethcnn_ldp_batch_run_device(ethcnn_ldp_batch* b, const ethcnn_ldp_batch_seq* seqs, int nseqs);
int ethcnn_ldp_batch_get_state(ethcnn_ldp_batch* b, int j, float* state_out, size_t nfloats /* nctu * 896 */);
int64_t ethcnn_ldp_batch_state_ctus(ethcnn_ldp_batch* b, int j);
int ethcnn_ldp_batch_set_chunk(ethcnn_ldp_batch* b, int frames);
int64_t ethcnn_ldp_batch_bytes(const int* widths, const int* heights, const int* nframes, int nseqs, int chunk_frames);
int ethcnn_ldp_batch_plan(const int* nctus, const int* nframes, int nseqs, int chunk_frames, int* fc_out, int* nchunks_out,
                          int* chunks_out /* [max_chunks][4] */, int max_chunks);
int ethcnn_ldp_set_thresholds_batch(ethcnn_ldp_batch* b, int j, float thr_l1_lower, float thr_l2_lower);
int ethcnn_ldp_clear_thresholds_batch(ethcnn_ldp_batch* b, int j);
int ethcnn_ldp_get_thresholds_batch(ethcnn_ldp_batch* b, int j, float* thr_l1_lower, float* thr_l2_lower, int* own);
/* ---- config #5 online, several live encoders: up to 32 SESSIONS on one context, each with a picture size and a resident recurrent state of
 *      its own; one call advances any subset of them by one frame.  The object holds up to 8 ETH-LSTM bundles, named by index per frame.
 *      DEFINITION: for every frame of a call, probs and the session's resident state EQUAL what ethcnn_ldp_step gives on a context of its
 *      own that holds the same CNN, that bundle and, as its thresholds, the session's RESOLVED pair, bit for bit, gates and their zero
 *      patterns (per 1024-CTU mini-batch of that session's own picture) included.  A session's resolved pair is its own when
 *      ethcnn_ldp_sessions_set_thresholds gave it one, else the context's pair as it stands when the call is made; the pair follows the
 *      session id, not the frame's place in the call, and no session's result depends on another's pair.  State rules of ethcnn_ldp_step: state_in is used when given, at ANY frame
 *      number (i_frame <= 1 included: the frame number then only carries the phase); without it a frame with i_frame <= 1 starts from
 *      zeros and a later one from the session's resident state (none resident: ETHCNN_ERR_ARG, in the wording of ethcnn_ldp_step).  Sessions that are not in a call keep their state.  The residual CNN and the stream
 *      are the context's; the context's own LSTM bundle and resident LDP state are neither used nor changed.
 *      What differs is the schedule: the CTU-load stage runs ONCE over a table of the call's pictures, in which picture j owns the 16-CTU
 *      groups [first_group_j, first_group_j + ceil(nctu_j / 16)) (rows of a short last group are padding that nothing reads), then trunk
 *      and FC1 run once over all groups -- cut at group boundaries into passes of at most the context's max_ctus_per_pass rows --, then
 *      ONE recurrence launch and ONE gate launch serve all frames of the call.
 *   ethcnn_ldp_sessions_create    nbundles bundle places on ctx (ETHCNN_ERR_ARG outside 1..8; text: ethcnn_last_error of the context).
 *                                 Destroy the object before its context.  Errors of every other entry: ethcnn_ldp_sessions_last_error.
 *   ethcnn_ldp_sessions_load_lstm_checkpoint / _load_lstm_blob / _load_lstm_synthetic / _get_lstm_blob   bundle i, as the batch's
 *   ethcnn_ldp_sessions_open      a session for width x height pictures; *session: its id, the lowest free one of 0..31 (ids are reused
 *                                 after ethcnn_ldp_sessions_close).  Allocates the session's state, roundup16(nctu) x 3584 bytes; may wait
 *                                 for the stream.  A 33rd open session is ETHCNN_ERR_ARG.
 *   ethcnn_ldp_sessions_close     forgets the session, its state and its gate pair (a reused id starts by inheriting the context's pair).
 *                                 Waits for nothing: work already enqueued for it completes.
 *   ethcnn_ldp_sessions_set_thresholds / _clear_thresholds / _get_thresholds   an OPEN session's gate pair, as
 *                                 ethcnn_ldp_set_thresholds_batch takes sequence index j's (a session that is not open: ETHCNN_ERR_ARG).
 *   ethcnn_ldp_sessions_step_device   n = 1..32 frames, each of another session.  Device pointers, asynchronous on the context's stream.
 *                                 Refused before anything is allocated or enqueued, every state left as it was: an open streamed call,
 *                                 no CNN weights, a bundle index that is out of range or empty (ETHCNN_ERR_NOWEIGHTS), a session that is
 *                                 not open or named twice, n outside 1..32, a null pointer, a pitch below the width, a state_in that is not
 *                                 16-byte aligned or a probs that is not 4-byte aligned, a probs that overlaps another frame's probs or
 *                                 any frame's state_in or picture, its own included (ETHCNN_ERR_ARG; the text names the frame).  luma and
 *                                 pitch need no alignment.  A call whose vectors do not fit fails with ETHCNN_ERR_NOMEM, states kept.  A
 *                                 failure after that point drops the states of the sessions in the call, and of no other.
 *   ethcnn_ldp_sessions_step      the same with HOST pointers (no alignment asked), synchronous: pictures and states are copied to the
 *                                 device, the probabilities back.  Every refusal above, ETHCNN_ERR_NOMEM included, comes before a
 *                                 caller's state is copied into the session's buffer.
 *   ethcnn_ldp_sessions_get_state the resident state of a session, float32 [nctu][2][448]; synchronous
 *   ethcnn_ldp_sessions_state_ctus   its CTU count; 0: none; negative: bad arguments
 *   ethcnn_ldp_sessions_bytes     host only, no context: what n open sessions that step together hold on the device,
 *                                 sum_j roundup16(nctu_j) x (1792 (vectors) + 3584 (state)); negative for bad arguments,
 *                                 a picture of more than 2^27 - 1 CTUs (what ethcnn_ldp_sessions_open refuses) among them.  Beside it: the
 *                                 bundle images and, for ethcnn_ldp_sessions_step, the staged pictures and probabilities.
 *   ethcnn_ldp_sessions_plan      host only: the layout of a call over pictures of these CTU counts, in the order given.
 *                                 first_group_out[j] = sum_{i<j} ceil(nctus_i / 16); the G = sum_j ceil(nctus_j / 16) groups are cut into
 *                                 *npasses_out passes of floor(cap / 16) groups, the last one shorter; pass_groups_out[p] (at most
 *                                 max_passes are written) is the group count of pass p.  cap = max_ctus_per_pass, 0 = the default of
 *                                 ethcnn_options (131072); below 16, n outside 1..32 or a CTU count below 1: ETHCNN_ERR_ARG.  Output
 *                                 pointers may be NULL. */
typedef struct ethcnn_ldp_sessions ethcnn_ldp_sessions;
typedef struct ethcnn_ldp_session_frame {
    int session;              /* id from ethcnn_ldp_sessions_open; at most once per call */
    const uint8_t* luma;      /* device (step_device) or host (step) */
    ptrdiff_t pitch;
    int qp, i_frame, bundle;
    const float* state_in;    /* may be NULL; 16-byte aligned on the device */
    float* probs;             /* [nctu][21] */
} ethcnn_ldp_session_frame;
int ethcnn_ldp_sessions_create(ethcnn_ctx* ctx, int nbundles, ethcnn_ldp_sessions** out);
void ethcnn_ldp_sessions_destroy(ethcnn_ldp_sessions* s);
const char* ethcnn_ldp_sessions_last_error(const ethcnn_ldp_sessions* s);
int ethcnn_ldp_sessions_bundles(const ethcnn_ldp_sessions* s);
int ethcnn_ldp_sessions_load_lstm_checkpoint(ethcnn_ldp_sessions* s, int bundle, const char* prefix);
int ethcnn_ldp_sessions_load_lstm_blob(ethcnn_ldp_sessions* s, int bundle, const float* blob, size_t nfloats);
int ethcnn_ldp_sessions_load_lstm_synthetic(ethcnn_ldp_sessions* s, int bundle, uint64_t seed, double head_gain);
int ethcnn_ldp_sessions_get_lstm_blob(ethcnn_ldp_sessions* s, int bundle, float* out, size_t nfloats);
int ethcnn_ldp_sessions_open(ethcnn_ldp_sessions* s, int width, int height, int* session);
int ethcnn_ldp_sessions_close(ethcnn_ldp_sessions* s, int session);
int ethcnn_ldp_sessions_step_device(ethcnn_ldp_sessions* s, const ethcnn_ldp_session_frame* frames, int n);
int ethcnn_ldp_sessions_step(ethcnn_ldp_sessions* s, const ethcnn_ldp_session_frame* frames, int n);
int ethcnn_ldp_sessions_get_state(ethcnn_ldp_sessions* s, int session, float* state_out, size_t nfloats /* nctu * 896 */);
int64_t ethcnn_ldp_sessions_state_ctus(ethcnn_ldp_sessions* s, int session);
int64_t ethcnn_ldp_sessions_bytes(const int* widths, const int* heights, int n);
int ethcnn_ldp_sessions_set_thresholds(ethcnn_ldp_sessions* s, int session, float thr_l1_lower, float thr_l2_lower);
int ethcnn_ldp_sessions_clear_thresholds(ethcnn_ldp_sessions* s, int session);
int ethcnn_ldp_sessions_get_thresholds(ethcnn_ldp_sessions* s, int session, float* thr_l1_lower, float* thr_l2_lower, int* own);
int ethcnn_ldp_sessions_plan(const int* nctus, int n, int max_ctus_per_pass, int* first_group_out, int* npasses_out, int* pass_groups_out,
                             int max_passes);
/* Pinned (page-locked) host memory: buffers a caller fills itself (file reads) and hands to the host entry points are
 * DMA-able directly, without the runtime's pageable staging copy.  ethcnn_ldp_step goes further: a luma / probs pointer that
 * lies inside such a buffer is read / written by the kernels IN PLACE (no copy launch at all); so does ethcnn_predict_luma for ONE
 * tightly packed picture (width % 16 == 0, up to 2304 CTUs): the launch pulls it over PCIe itself while it computes.  Buffers still allocated when
 * the context is destroyed are freed with it. */
int ethcnn_host_alloc(ethcnn_ctx* ctx, size_t bytes, void** out);
int ethcnn_host_free(ethcnn_ctx* ctx, void* p);

/* ---- host budget (multi-GPU): one process per GPU, and every process fills its pinned staging ring with a
 *      pool of host threads.  The node's CPU budget (cgroup quota, else logical CPUs / 2) is DIVIDED by the number of
 *      predictor processes on the node (env ETHCNN_LOCAL_WORKERS, else torchrun's LOCAL_WORLD_SIZE, else 1), capped at 16.
 *      ethcnn_host_thread_budget is pure (no context, no device): usable <= 0 probes the box. */
int ethcnn_host_thread_budget(int local_workers, int usable_cpus);
int ethcnn_host_threads(ethcnn_ctx* ctx); /* the pool size this context uses */

/* ---- device plumbing for callers without a HIP binding (ctypes, cgo, JNI ...) */
int ethcnn_device_alloc(ethcnn_ctx* ctx, size_t bytes, void** out);
int ethcnn_device_free(ethcnn_ctx* ctx, void* p);
int ethcnn_memcpy_h2d(ethcnn_ctx* ctx, void* dst, const void* src, size_t bytes);
int ethcnn_memcpy_d2h(ethcnn_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Waits for everything enqueued on the context's main stream.  When the LAST thing enqueued is a single-launch pass or an LDP
 * step, the wait is a spin on a completion word in page-locked memory that the launch's last block stores (about 5 us sooner
 * than hipStreamSynchronize; bounded, with hipStreamSynchronize as the fallback, which also reports device faults); otherwise it
 * is hipStreamSynchronize.  Env ETHCNN_DONE_WORD=0: always the latter. */
int ethcnn_synchronize(ethcnn_ctx* ctx);
int ethcnn_device_name(const ethcnn_ctx* ctx, char* out, size_t cap);
/* Cold start (no reference counterpart; the reference quotes "1~10 s" of TensorFlow initialisation, README.md:124): how long
 * ethcnn_create took, and how much of it was its first HIP call (loading and initialising the runtime).  Milliseconds. */
int ethcnn_get_startup_times(const ethcnn_ctx* ctx, double* runtime_init_ms, double* create_ms);

/* ---- measurement: per-stage kernel time from HIP events recorded on the ctx stream
 *      (replaces the reference's only instrument, the 'Predicting Time' wall clock,
 *      video_to_cu_depth.py:142-145). */
enum {
    ETHCNN_STAGE_TILE = 0,  /* k0: CTU load + zero-pad tiling + integer pooling (HBM-bound) */
    ETHCNN_STAGE_TRUNK = 1, /* k1: mean removal + 3 conv stages x 21 units (MFMA)          */
    ETHCNN_STAGE_FC1 = 2,   /* k2: [N,2688]x[2688,448] (MFMA) -- dominant kernel           */
    ETHCNN_STAGE_HEADS = 3, /* k3: FC2 + FC3 + sigmoid of the three heads, fused (MFMA)    */
    ETHCNN_STAGE_GATE = 4,  /* k5: batch-level gates (zero fill)                           */
    ETHCNN_NSTAGES = 5
};
typedef struct ethcnn_stage_times {
    double ms[ETHCNN_NSTAGES];       /* accumulated kernel time per stage since reset */
    int64_t launches[ETHCNN_NSTAGES];
    int64_t ctus;                    /* CTUs processed since reset */
    int64_t timed[ETHCNN_NSTAGES];   /* launches whose time is in ms[] (level 1 samples every 3rd FC1 stage) */
    int64_t timed_ctus[ETHCNN_NSTAGES]; /* CTUs of those launches: rate = work(timed_ctus) / ms */
    int64_t timing_errors;           /* event create/record/elapsed failures: those launches are not in ms[]/timed[] */
} ethcnn_stage_times;
int ethcnn_set_profiling(ethcnn_ctx* ctx, int level); /* 0 off; 1 events around the dominant kernel (FC1) on every 3rd
                                                          pass (an event pair costs ~12 us of stream time); 2 around every launch */
int ethcnn_get_stage_times(ethcnn_ctx* ctx, ethcnn_stage_times* out); /* synchronizes */
/* Pass pipeline (default on): the CTU-load stage of pass i+1 runs on a side stream beside FC1 of pass i (consecutive passes
 * of one call, or consecutive asynchronous ethcnn_predict_luma_device calls).  Results do not depend on it.  Off = every
 * stage of every pass in order on one stream: what per-stage timings (profiling level 2) should be read against, because
 * with the pipeline on the stage intervals overlap.  Synchronizes.  Environment: ETHCNN_OVERLAP=0 starts contexts with it off. */
int ethcnn_set_pass_pipeline(ethcnn_ctx* ctx, int on);
int ethcnn_reset_stage_times(ethcnn_ctx* ctx);
/* Arithmetic plan of the big (multi-launch) All-Intra passes.  FC1 ([N,2688] x
 * [2688,448]) is 78 % of the path's arithmetic and the exact-fp32 MFMA runs at 1/16 of the 16-bit matrix rate.
 *   0 (default)  exact fp32 on v_mfma_f32_16x16x4_f32: every result of the library is bit-identical to oracle/ethcnn_oracle.c;
 *   2 ("fast", FC1 as fp16 x 2)  passes that take the multi-launch path (more than 2304 CTUs, or rows that are not 16-byte
 *                aligned) run FC1 on the 16-bit matrix pipe: both operands as TWO fp16 pieces of the power-of-two scaled fp32 value
 *                (h0 + h1 represents it to 2^-24 relative; the feature scale comes from a bound derived from the conv weights at
 *                load, not from observation, so no piece can overflow), THREE products, fp32 accumulation;
 *   3 ("fast", everything as fp16 x 2)  plan 2, and the trunk's three conv layers (ethcnn_trunk_fast.hip: conv1 on the exact integer
 *                pixel sums -- its weight pieces carry the pixel scale and its accumulators start at the mean-removal constant, so no
 *                arithmetic per output beyond the leaky-ReLU --, conv2 / conv3 with fp16 x 2 splits; the CTU-load
 *                stage is folded into the trunk: one pass over the luma frames, no pixel records in HBM) and the heads' FC2 / FC3
 *                (ethcnn_heads_fast.hip, scaled residual pieces) on the 16-bit pipe as well.  The fastest plan.
 *   (1 was round 4's bf16 x 3 form of FC1; removed in round 5 -- slower than plan 2 and no more accurate -- and now an argument error.)
 * Measured against float64 these sums are as accurate as plan 0's fmaf chains (profiles/r04_bf16x3_probe.txt: the error of a 2688-
 * term fp32 sum is set by the roundings of its accumulation), but the ORDER of the fp32 additions differs, so probabilities agree
 * with plan 0 / the oracle to about 1e-6..1e-5, not bit for bit (tests: <= 1e-4, the north star's tolerance; thresholded decisions may
 * differ on knife edges only).  The batch gates are computed exactly in every plan.  The single-launch small pass and the LDP path
 * always use plan 0 -- which includes ONE picture handed to ethcnn_predict_luma (the host entry's latency path: a picture with 16-byte
 * aligned rows runs as single-launch passes, whole or in 1024-CTU pieces): the plans show in ethcnn_predict_luma_device, the file /
 * multi-frame host entries and the streamed entries of pictures above 2304 CTUs (tests/test_gpu_fast_plan.py).  Env ETHCNN_FC1_PLAN=2|3 starts contexts in that plan.  Takes effect with the next pass enqueued. */
int ethcnn_set_fc1_plan(ethcnn_ctx* ctx, int plan);
int ethcnn_get_fc1_plan(const ethcnn_ctx* ctx);
/* Load-time accuracy guard of plans 2 / 3.  The pieces of a split value are exact to 2^-24 relative only while the value stays within
 * about 2^12 of the GUARANTEED bound its scale was derived from; below that an absolute floor takes over.  Seeded and well-conditioned
 * trained weights are far inside; a checkpoint with a few outlier weights (a bound 10^3..10^9 above typical values) is not.  At the
 * first pass under a plan (and here, on request) the library pushes every such floor of the plan through the |weights| of the layers
 * behind it -- all errors aligned, activations always at their floor -- down to the probabilities: a rigorous upper bound, computed from
 * the weights alone (video_to_cu_depth.py:126-133: any of the four checkpoints a run may restore must be safe).  At or below 2.5e-5 (a
 * quarter of the 1e-4 contract) the plan is accepted on the bound alone.  Above it the worst case decides nothing (it is pessimistic by
 * the looseness of the very bounds it guards), so the plan is MEASURED once: a seeded calibration picture (640 CTUs: flat, low-contrast,
 * gradient, noise, edge and texture tiles) through the exact plan and through the plan at QP 22 and QP 37, gates open; max |dp| <= 2.5e-5 accepts, anything
 * else REFUSES: the pass returns ETHCNN_ERR_PLAN_REFUSED with the numbers in ethcnn_last_error, nothing is computed, the context stays
 * usable (ethcnn_set_fc1_plan(ctx, 0 or 2)).  Never a silent loss of accuracy, never a silent fallback.  ~3 ms, once per weight load.
 * The measured stage is empirical -- one synthetic picture -- so a deployment checks a plan on its OWN content with ethcnn_audit_plan_device
 * / ethcnn_audit_plan_yuv_file ("comparing two predictions" below).
 * Weights that are not finite (a NaN or an infinity anywhere in the blob, e.g. a diverged training run's export) are REFUSED before
 * either stage, unmeasured (*apriori_bound = +Inf, *measured < 0): they have no fp16 scale.  Plan 0 computes them as the reference
 * arithmetic does (NaN probabilities, which the analysis tools reject).
 *   ethcnn_check_fc1_plan  ETHCNN_OK / ETHCNN_ERR_PLAN_REFUSED for the loaded weights; *apriori_bound, *measured (may be NULL; measured
 *                           < 0: the bound sufficed and nothing was run).
 * The launchers (video_to_cu_depth.py, tools/video_to_cu_depth.c) call it when ETHCNN_FC1_PLAN is set and continue with plan 0 after
 * printing the refusal. */
int ethcnn_check_fc1_plan(ethcnn_ctx* ctx, int plan, double* apriori_bound /* may be NULL */, double* measured /* may be NULL */);
/* the a-priori bound for a blob in host memory: no context, no device (pure host arithmetic).  ETHCNN_OK: the bound alone accepts */
int ethcnn_fast_plan_bound(const float* blob, size_t nfloats, int plan, double* prob_err_bound, double* feature_bound /* may be NULL */);
/* Single-launch small pass (default on): a pass of <= 2304 CTUs (up to one 3840x2160 picture) whose rows are 16-byte aligned (width, pitch, frame stride and
 * base pointer multiples of 16) -- one picture from the in-process encoder hook, every Low-Delay-P frame, the reference's own
 * 768x512 case -- runs CTU load + trunk -> FC1 -> heads -> gates as ONE kernel launch (a dataflow inside one grid, per-group /
 * per-tile completion counters; csrc/ethcnn_small.hip) instead of five dependent launches; the LDP front-end
 * (ethcnn_resi_vectors*) likewise as one launch instead of three.  Time is booked under ETHCNN_STAGE_FC1.  Off, or for other
 * geometries: the tile / trunk / FC1 / heads / gate launches.  Results do not depend on it.  Env: ETHCNN_SMALL=0. */
int ethcnn_set_small_pass_launch(ethcnn_ctx* ctx, int on);

/* Box calibration (no reference counterpart): what THIS GPU sustains in exact-fp32 MFMAs (v_mfma_f32_16x16x4_f32, nothing
 * else issued) over about `seconds` (0 < seconds <= 5) of pure matrix work, in TFLOP/s.  bench.py prints it beside the
 * roofline: boxes of one pool differ by several per cent in sustained clock, the data-sheet peak (157.3) does not. */
int ethcnn_measure_mfma_rate(ethcnn_ctx* ctx, double seconds, double* tflops);

/* ---- parity-test introspection: intermediates of the LAST pass, copied to host. */
enum {
    ETHCNN_DBG_FEATURES = 0, /* [n][2688] h_conv_flat (net_CNN.py:150)          */
    ETHCNN_DBG_FC1 = 1,      /* [n][448]  h_fc1_64|32|16 after leaky-ReLU       */
    ETHCNN_DBG_FC2 = 2,      /* [n][336]  h_fc2_64|32|16 after leaky-ReLU       */
    ETHCNN_DBG_LOGITS = 3,   /* [n][21]   pre-sigmoid                           */
    ETHCNN_DBG_RAW_PROBS = 4 /* [n][21]   before the gates                      */
};
int ethcnn_debug_fetch(ethcnn_ctx* ctx, int which, float* host_out, size_t nfloats);
/* FC2 / LOGITS / RAW_PROBS are only stored when capture is on (off by default: 1.7 KB/CTU of HBM
 * writes nobody reads in production); FEATURES and FC1 are the path's own buffers, always there. */
int ethcnn_set_debug_capture(ethcnn_ctx* ctx, int on);

/* ---- checkpoint introspection (the TF-V2 bundle reader on its own; used by the loader
 *      above and by the known-answer tests against the reference's .index files). */
typedef struct ethcnn_ckpt_entry {
    char name[64];
    int dtype, rank;       /* dtype 1 = DT_FLOAT */
    int64_t shape[4];
    int shard;
    int64_t offset, size;  /* bytes, into <prefix>.data-<shard>-of-<n> */
    uint32_t crc32c;       /* masked, as stored */
} ethcnn_ckpt_entry;
int ethcnn_ckpt_read_index(const char* index_path, ethcnn_ckpt_entry* entries, int cap, int* n_out,
                           char* err, size_t errcap);
uint32_t ethcnn_crc32c_masked(const void* data, size_t nbytes);
/* <prefix>.index + <prefix>.data-00000-of-00001 -> blob (crc-checked); no context / device needed */
int ethcnn_ckpt_read_blob(const char* prefix, float* blob_out, size_t nfloats, char* err, size_t errcap);
int ethcnn_ckpt_read_lstm_blob(const char* prefix, float* blob_out, size_t nfloats, char* err, size_t errcap);


/* TF-V2 bundle WRITER (tf.train.Saver's format, BundleWriter layout): blob -> <prefix>.index + <prefix>.data-00000-of-00001, each
 * written to a temp file and renamed.  What ethcnn_load_checkpoint and both launchers restore.  No context / device needed. */
int ethcnn_ckpt_write_blob(const char* prefix, const float* blob, size_t nfloats, char* err, size_t errcap);
/* the same writer over the 18-tensor ETH-LSTM table (ETHCNN_LSTM_BLOB_FLOATS floats): what ethcnn_load_lstm_checkpoint restores */
int ethcnn_ckpt_write_lstm_blob(const char* prefix, const float* blob, size_t nfloats, char* err, size_t errcap);

/* ---- training (All-Intra ETH-CNN; ETH-CNN_Training_AI/net_CTU64.py:94-206 + train_CNN_CTU64.py:36-47; the Low-Delay-P
 *      residual CNN as a variant, see "net = ETHCNN_TRAIN_NET_LDP" below).
 *      A trainer is bound to a context: its device and its stream.  Everything a step computes runs in hand-written gfx950 kernels
 *      (exact fp32; csrc/ethcnn_train.h lists the 8 launches of a step).  Deterministic: same weights, data, seed and calls ->
 *      bit-identical weights.
 *   Samples: the reference's record format (input_data.py:16,92-116), 4992 bytes = 4096 luma + 64 pad + 52 x 16 label bytes; the
 *      label row of QP q is at byte 4160 + 16 q.  Set 0 = training, 1 = validation; uploaded once, resident in HBM.
 *   Batches drawn on the device (ethcnn_train_run), with mix(z) = splitmix64's output function
 *      (z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31) and
 *      draw(stream, step, slot, unit) = mix(mix(mix(seed ^ stream * 0xD1B54A32D192ED03) ^ step) ^ (slot << 12 | unit)) (uint64):
 *        sample index of batch slot b   = (draw(1, step, b, 0) >> 32) * n_train >> 32      (uniform, with replacement)
 *        QP of batch slot b             = qps[(draw(2, step, b, 0) >> 32) * nqps >> 32]
 *        dropout keep of unit u         = (draw(3, step, b, u) >> 40) * 2^-24 < keep   (float compare; u = 0..447 FC1 in head order
 *                                         64|32|16 with keep 0.5, u = 448 + 0..335 FC2 with keep 0.8; kept values scaled by 1 / keep)
 *      `step` is the 1-based global step, which also sets the learning rate: lr_init * decay_rate ^ floor(step / decay_steps).
 *   Optimiser: MomentumOptimizer without Nesterov, accum = momentum * accum + grad; w -= lr * accum.  The blob (key order, as in the
 *      checkpoints) is the master copy of the weights.
 *   net = ETHCNN_TRAIN_NET_LDP: the Low-Delay-P residual CNN (ETH-CNN_Training_LDP/net_CTU64.py:94-209, train_resi_CNN_CTU64.py),
 *      whose checkpoint is model_LDP_2000000_qp22~37.dat.  Same graph, loss, labels, dropout and schedule; it differs in:
 *        records: 16516 bytes (input_data.py:48-50) = 64 header bytes, then 4 slots of 4113 bytes = [QP byte | 16 label bytes |
 *          4096 residual bytes] at 64 + 4113 s.  ethcnn_train_set_samples returns ERR_FORMAT if nbytes % 16516 != 0, or if any record's
 *          four slot QP bytes differ from record 0's (four distinct values in 0..51; the message names the first such record).
 *        QPs: a sample at QP q reads the slot whose QP byte is q (its labels and residual).  Uploading the training set sets the QP
 *          list to its four slot QPs (the reference trains every MODEL_TYPE on all four); ethcnn_train_set_qps may choose a subset
 *          (single-QP training), any other QP is ERR_ARG, as it is in explicit batches and in evaluation.  The device-drawn QP uses
 *          the formula above, so a uniform draw over the four slots is input_data.py:119-130's numpy.random.choice(4).
 *        input scaling: x = (x - 128) / 255 * 10 and the FC2 / FC3 QP feature qp / 51 * 0.18 (fp32, in that order).
 *        initial biases: truncated normal sigma 0.1 like the weights (net_CTU64.py:38-40).
 *        evaluation at qp = -1 (LDP only): sample i of the n evaluated is at the slot draw(2, 0, i, 0) picks,
 *          slot = (draw(2, 0, i, 0) >> 32) * 4 >> 32 -- the reference's mixed-QP 5000-sample evaluation.
 *   tune 1..3 (PARTLY_TUNING_MODE, net_CTU64.py:200-209; either net): only the six FC tensors of head 64 / 32 / 16 are optimised;
 *      every other weight and its momentum accumulator stay bit-identical.  Such a step skips the trunk backward, and
 *      ETHCNN_TRAIN_DBG_GRADS holds the tuned head's tensors only (the others keep whatever was there).  Checkpoints hold all 36. */
typedef struct ethcnn_trainer ethcnn_trainer;
typedef struct ethcnn_train_options {
    int batch;           /* samples per step (reference: 64)                                   */
    float lr_init;       /* 0.01                                                               */
    float momentum;      /* 0.9                                                                */
    float decay_rate;    /* 0.3163                                                             */
    int64_t decay_steps; /* 250000                                                             */
    int dropout;         /* 1: isdrop = 1 in training steps (evaluation never drops)           */
    uint64_t seed;       /* the draw() seed of batches and dropout masks                       */
    int net;             /* ETHCNN_TRAIN_NET_AI (0) or ETHCNN_TRAIN_NET_LDP (1); else ERR_ARG   */
    int tune;            /* PARTLY_TUNING_MODE 0..3: 0 all tensors, 1/2/3 only head 64/32/16   */
    int reserved[6];
} ethcnn_train_options;
enum { ETHCNN_TRAIN_NET_AI = 0, ETHCNN_TRAIN_NET_LDP = 1 };
enum { ETHCNN_TRAIN_SET_TRAIN = 0, ETHCNN_TRAIN_SET_VALID = 1 };
enum {
    ETHCNN_TRAIN_DBG_GRADS = 0,     /* [1288210] gradient of the last step, blob layout                        */
    ETHCNN_TRAIN_DBG_MASK_FC1 = 1,  /* [batch][448] dropout keep (0 / 1) of the last step, heads 64|32|16      */
    ETHCNN_TRAIN_DBG_MASK_FC2 = 2,  /* [batch][336]                                                            */
    ETHCNN_TRAIN_DBG_PROBS = 3,     /* [batch][21] probabilities of the last step                              */
    ETHCNN_TRAIN_DBG_INDICES = 4,   /* [batch][2] (sample index, QP) of the last step, as floats               */
    ETHCNN_TRAIN_DBG_ACCUM = 5,     /* [1288210] momentum accumulators                                         */
    ETHCNN_TRAIN_DBG_H1 = 6         /* [batch][448] leaky-ReLU FC1 outputs of the last step, before dropout    */
};
int ethcnn_train_create(ethcnn_ctx* ctx, const ethcnn_train_options* opt, ethcnn_trainer** out);
void ethcnn_train_destroy(ethcnn_trainer* tr); /* before ethcnn_destroy of its context */
/* tf.truncated_normal(stddev 0.1) weights (|x| <= 0.2, redrawn beyond), tf.constant(0.01) biases (net_CTU64.py:37-43; LDP: biases
 * truncated normal too, from the same generator); our RNG, seeded; accumulators zeroed */
int ethcnn_train_init_weights(ethcnn_trainer* tr, uint64_t seed);
int ethcnn_train_set_blob(ethcnn_trainer* tr, const float* blob, const float* accum /* NULL = zeros */, size_t nfloats);
int ethcnn_train_get_blob(ethcnn_trainer* tr, float* blob, float* accum /* may be NULL */, size_t nfloats);
int ethcnn_train_set_samples(ethcnn_trainer* tr, int set, const uint8_t* records, size_t nbytes); /* ERR_FORMAT: nbytes % 4992 (LDP 16516) */
int ethcnn_train_set_qps(ethcnn_trainer* tr, const int* qps, int nqps);                           /* SELECT_QP_LIST, 0..51 (LDP: slot QPs) */
/* steps first_step .. first_step + nsteps - 1 with device-drawn batches; asynchronous (nothing read back) */
int ethcnn_train_run(ethcnn_trainer* tr, int64_t first_step, int64_t nsteps);
/* loss_list / accuracy_list (64, 32, 16) of the last step enqueued; waits for it */
int ethcnn_train_last_stats(ethcnn_trainer* tr, float loss3[3], float acc3[3]);
/* one step on an explicit batch of n == batch training samples (tests); synchronous */
int ethcnn_train_step_indices(ethcnn_trainer* tr, int64_t step, const int32_t* idx, const int* qp, int n, float loss3[3], float acc3[3]);
/* forward only (no dropout) over n samples of a set at one QP (idx NULL: samples 0 .. n-1); the loss and accuracy lists are those of
 * ONE batch of all n samples (train_CNN_CTU64.py's 5000-sample sess.run), not a mean over pieces.  probs [n][21] may be NULL.
 * LDP: qp is a slot QP of the set, or -1 for the per-sample slot draw above. */
int ethcnn_train_evaluate(ethcnn_trainer* tr, int set, const int32_t* idx, int64_t n, int qp, float loss3[3], float acc3[3], float* probs);
int ethcnn_train_debug_fetch(ethcnn_trainer* tr, int which, float* out, size_t nfloats);
const char* ethcnn_train_last_error(const ethcnn_trainer* tr);

/* ---- training, several models at once: a trainer GROUP is k (1..8) independent trainers of "training" above that share a context,
 *      its stream, the two resident sample sets and every launch of a step.  A deployment of the All-Intra predictor needs four models
 *      (model_2000000_qp20~25 .. qp35~40) that differ only in the QP list and read the same sample file; several seeds or learning
 *      rates of one model are the other use.  A step of the group is still 8 launches (tune 1..3: 7), each over all members
 *      (csrc/ethcnn_train.h "trainer group"); an evaluation is still launches 1-3 over pieces, then one loss launch.
 *   Exactness: member m computes what ethcnn_train_* computes for a trainer with opts[m], its weights, its QP list and the same
 *      samples -- bit for bit, whatever k is and wherever in the group the member sits.  The members share the records and nothing
 *      else: each has its own weights, accumulators, RNG streams (opts[m].seed), batch-global label counts and learning rate.
 *   Members of one group have the same net, batch and tune; they may differ in seed, lr_init, momentum, decay_rate, decay_steps and
 *      dropout.  ethcnn_train_group_check (host only, no context) returns ETHCNN_ERR_ARG and a message that names the member and
 *      the field for anything else, and for an option ethcnn_train_create refuses; err may be NULL.
 *   Arrays over members are member-major: seeds[k], qps[k], loss[k][3], acc[k][3], idx[k][batch], qp[k][batch], probs[k][n][21].
 *   A member index outside 0..k-1 is ETHCNN_ERR_ARG. */
typedef struct ethcnn_train_group ethcnn_train_group;
int ethcnn_train_group_check(const ethcnn_train_options* opts, int k, char* err, size_t errcap);
int ethcnn_train_group_create(ethcnn_ctx* ctx, const ethcnn_train_options* opts, int k, ethcnn_train_group** out);
void ethcnn_train_group_destroy(ethcnn_train_group* grp); /* before ethcnn_destroy of its context */
int ethcnn_train_group_init_weights(ethcnn_train_group* grp, const uint64_t* seeds /* [k] */); /* member m: ethcnn_train_init_weights(seeds[m]) */
int ethcnn_train_group_set_blob(ethcnn_train_group* grp, int member, const float* blob, const float* accum /* NULL = zeros */, size_t nfloats);
int ethcnn_train_group_get_blob(ethcnn_train_group* grp, int member, float* blob, float* accum /* may be NULL */, size_t nfloats);
/* ONE copy in HBM for all members; LDP: the slot-QP pass runs once and every member's QP list becomes the four slots */
int ethcnn_train_group_set_samples(ethcnn_train_group* grp, int set, const uint8_t* records, size_t nbytes);
int ethcnn_train_group_set_qps(ethcnn_train_group* grp, int member, const int* qps, int nqps);
/* steps first_step .. first_step + nsteps - 1 of every member, device-drawn batches; asynchronous (nothing read back) */
int ethcnn_train_group_run(ethcnn_train_group* grp, int64_t first_step, int64_t nsteps);
int ethcnn_train_group_last_stats(ethcnn_train_group* grp, float* loss /* [k][3] */, float* acc /* [k][3] */);
/* one step on explicit batches, n == batch samples per member: idx [k][n], qp [k][n]; synchronous */
int ethcnn_train_group_step_indices(ethcnn_train_group* grp, int64_t step, const int32_t* idx, const int* qp, int n, float* loss, float* acc);
/* every member evaluates the same n samples (idx NULL: 0 .. n-1), member m at qps[m] (LDP: a slot QP or -1, the slot draw with the
 * member's seed); each member's loss and accuracy lists are those of ONE batch of all n.  probs [k][n][21] may be NULL. */
int ethcnn_train_group_evaluate(ethcnn_train_group* grp, int set, const int32_t* idx, int64_t n, const int* qps /* [k] */, float* loss,
                                float* acc, float* probs);
int ethcnn_train_group_debug_fetch(ethcnn_train_group* grp, int member, int which, float* out, size_t nfloats);
const char* ethcnn_train_group_last_error(const ethcnn_train_group* grp);

/* ---- ETH-LSTM training (ETH-LSTM_Training_LDP/net_CTU64.py:85-276, input_data.py:88-147, train_LSTM_CTU64.py:42-52): the 20-step
 *      unrolled LSTM of the Low-Delay-P path with back-propagation through time, one model per QP (model_LDP_200000_qp<QP>.dat).
 *      Mirrors ethcnn_train_* one to one; bound to a context (its device and stream); hand-written gfx950 kernels, exact fp32,
 *      deterministic (csrc/ethcnn_lstm_train.h lists the 10 launches of a step).  The blob is the 18-tensor LSTM table
 *      (ETHCNN_LSTM_BLOB_FLOATS floats, key order), the master copy of the weights.
 *   Samples: 37264 bytes = 64 info bytes + 20 time slots of 465 float32 [qp | 16 depth labels | 448-vector of the residual CNN]
 *      (input_data.py:94-108).  Slot 0 is the current frame, slot k frame i - k; i_frame is the little-endian u32 at info byte 10 and
 *      i_frame_in_GOP[k] = (i_frame - k) mod 4 (non-negative, as numpy.mod; so a GOP value outside 0..3 cannot arise, and a sample
 *      with i_frame < 19, which get_LSTM_input.py never writes, is accepted with positions wrapped below frame 0).
 *      ethcnn_lstm_train_set_samples returns ERR_FORMAT if nbytes % 37264 != 0, or (one pass
 *      on the device) if a kept sample has a QP that is not an integer in 0..51, a label that is not an integer in 0..3 or a non-finite
 *      vector element.  ethcnn_lstm_train_set_qps BEFORE an upload selects by QP (SELECT_QP_LIST, input_data.py:126-134): only the
 *      samples whose slot-0 QP is in the list are kept, in file order, and sample indices count the kept ones (n = 0: keep all).
 *   Graph as shipped: three cells (hidden 64 / 128 / 256 on vector columns [0,64) / [64,192) / [192,448); forget_bias 1, cell_clip 5,
 *      gates i, j, f, o, zero initial state) consume slot 19 first and slot 0 last; the prediction of slot p is the one computed when
 *      slot p was the input.  The external features are NOT reversed: the heads of the step that reads slot p get the QP and the GOP
 *      one-hot of slot 19 - p (net_CTU64.py:125 indexes both lists by the unrolled step).  This is how the shipped models were
 *      trained; it is transcribed, not corrected.  Heads: fc2([h, qp, onehot4]) leaky-ReLU(0.2), fc3([h2, qp, onehot4]) sigmoid.
 *      Rows of every per-row output: r = 20 b + p (sample b of the batch, slot p).  Labels, class-balanced loss with counts over all
 *      20 x batch rows, accuracy: net_CTU64.py:160-176, 220-233, 263-271.
 *   qp_scale: the QP feature is qp / 51 * qp_scale.  0 means 1.0, the training script as shipped (net_CTU64.py:149).  The deployed
 *      one-step graph -- ethcnn_lstm_step_device and both LDP daemons -- uses qp / 51 * 0.18, so a model meant for them is trained
 *      with qp_scale = 0.18; one trained with 1.0 sees a shifted feature there.
 *   Dropout (training steps with dropout = 1 only): keep 0.5 on the cell OUTPUT fed to fc2 (the h carried in the state is not
 *      dropped), keep 0.8 on fc2's output; kept values scaled by 1 / keep.
 *   RNG: draw() of "training" above with three more streams:
 *        sample index of batch slot b  = (draw(4, step, b, 0) >> 32) * n_train >> 32            (next_batch_random: with replacement)
 *        keep of unit u of row r       = (draw(5, step, r, u) >> 40) * 2^-24 < keep   (u = 0..447 cell outputs 64|32|16, keep 0.5;
 *                                        u = 448 + 0..335 fc2 outputs, keep 0.8)
 *        initial weight k of tensor t  = (2 * (draw(6, t, 0, k) >> 11) * 2^-53 - 1) * limit  (t: index in the table, key order)
 *      limit: tf.get_variable's default glorot_uniform, sqrt(6 / (fan_in + fan_out)) for the six matrices and three LSTM kernels,
 *      sqrt(3 / n) for the six fc biases (1-D [n]: fan_in = fan_out = n); the LSTM biases start at zero.
 *   Optimiser: gradients of loss_16 + loss_32 + loss_64, tf.clip_by_global_norm(., clip_norm) (scale = clip * min(1 / norm,
 *      1 / clip); clip_norm 0: no clip), MomentumOptimizer, lr = lr_init * decay_rate ^ floor(step / decay_steps).  The cell clip's
 *      gradient is zero where c was clipped.  The global norm is summed in a fixed two-level order (512 ranges, then their sums). */
typedef struct ethcnn_lstm_trainer ethcnn_lstm_trainer;
typedef struct ethcnn_lstm_train_options {
    int batch;           /* samples per step (reference: 64), 1..4096                          */
    float lr_init;       /* 0.1                                                                */
    float momentum;      /* 0.9                                                                */
    float decay_rate;    /* 0.3163                                                             */
    int64_t decay_steps; /* 25000                                                              */
    int dropout;         /* 1: isdrop = 1 in training steps (evaluation never drops)           */
    uint64_t seed;       /* the draw() seed of batches and dropout masks                       */
    float qp_scale;      /* 0 = 1.0 (as shipped); 0.18 for a model the daemons will run        */
    float clip_norm;     /* MAX_GRAD_NORM = 5; 0 = no clip                                     */
    int reserved[6];
} ethcnn_lstm_train_options;
#define ETHCNN_LSTM_SAMPLE_BYTES 37264
enum {
    ETHCNN_LSTM_DBG_GRADS = 0,    /* [760078] gradient of the last step BEFORE the clip, blob layout                        */
    ETHCNN_LSTM_DBG_NORM = 1,     /* [1] its global norm                                                                    */
    ETHCNN_LSTM_DBG_ACCUM = 2,    /* [760078] momentum accumulators                                                         */
    ETHCNN_LSTM_DBG_MASK_H = 3,   /* [rows][448] keep (0 / 1) of the cell outputs, last step                                */
    ETHCNN_LSTM_DBG_MASK_FC2 = 4, /* [rows][336]                                                                            */
    ETHCNN_LSTM_DBG_PROBS = 5,    /* [20 batch][21] probabilities of the last step                                          */
    ETHCNN_LSTM_DBG_INDICES = 6,  /* [rows / 20] sample indices, as floats                                                  */
    ETHCNN_LSTM_DBG_STATE_C = 7,  /* [rows][448] c (after the clip) computed with slot p as the input, cells 64|32|16        */
    ETHCNN_LSTM_DBG_STATE_H = 8   /* [rows][448] h (not dropped)                                                            */
};  /* rows = 20 x the samples of the last step, or of the last piece (<= max(batch, 256) samples) of the last evaluation:
     ethcnn_lstm_train_debug_rows */
int ethcnn_lstm_train_create(ethcnn_ctx* ctx, const ethcnn_lstm_train_options* opt, ethcnn_lstm_trainer** out);
void ethcnn_lstm_train_destroy(ethcnn_lstm_trainer* tr); /* before ethcnn_destroy of its context */
int ethcnn_lstm_train_init_weights(ethcnn_lstm_trainer* tr, uint64_t seed); /* accumulators zeroed */
int ethcnn_lstm_train_set_blob(ethcnn_lstm_trainer* tr, const float* blob, const float* accum /* NULL = zeros */, size_t nfloats);
int ethcnn_lstm_train_get_blob(ethcnn_lstm_trainer* tr, float* blob, float* accum /* may be NULL */, size_t nfloats);
int ethcnn_lstm_train_set_qps(ethcnn_lstm_trainer* tr, const int* qps, int nqps); /* applies to the uploads that follow */
int ethcnn_lstm_train_set_samples(ethcnn_lstm_trainer* tr, int set, const uint8_t* records, size_t nbytes);
int64_t ethcnn_lstm_train_num_samples(const ethcnn_lstm_trainer* tr, int set); /* kept samples of a set */
/* steps first_step .. first_step + nsteps - 1 with device-drawn batches; asynchronous (nothing read back) */
int ethcnn_lstm_train_run(ethcnn_lstm_trainer* tr, int64_t first_step, int64_t nsteps);
int ethcnn_lstm_train_last_stats(ethcnn_lstm_trainer* tr, float loss3[3], float acc3[3]);
/* one step on an explicit batch of n == batch training samples (tests); synchronous */
int ethcnn_lstm_train_step_indices(ethcnn_lstm_trainer* tr, int64_t step, const int32_t* idx, int n, float loss3[3], float acc3[3]);
/* forward only (no dropout, no update) over n samples of a set (idx NULL: samples 0 .. n-1); the loss and accuracy lists are those
 * of ONE batch of all n samples (train_LSTM_CTU64.py's NUM_TRAIN_PART = 10000 sess.run): the balanced loss divides by batch-global
 * counts, so a mean over pieces would be another number.  probs [20 n][21] may be NULL.  Meant for a call every 1000 steps, not
 * for a tight loop: each call allocates and frees its three [20 n] device arrays, and every piece's projection GEMM runs over the
 * full max(batch, 256) x 20 rows (rows past a short piece hold an earlier batch's vectors; they are computed and never read). */
int ethcnn_lstm_train_evaluate(ethcnn_lstm_trainer* tr, int set, const int32_t* idx, int64_t n, float loss3[3], float acc3[3], float* probs);
int ethcnn_lstm_train_debug_fetch(ethcnn_lstm_trainer* tr, int which, float* out, size_t nfloats);
int64_t ethcnn_lstm_train_debug_rows(const ethcnn_lstm_trainer* tr); /* `rows` of the per-row debug buffers right now */
const char* ethcnn_lstm_train_last_error(const ethcnn_lstm_trainer* tr);

/* ---- ETH-LSTM training, several models at once: an LSTM trainer GROUP is k (1..8) independent trainers of "ETH-LSTM training" above
 *      that share a context, its stream, ONE copy of each resident sample set and every launch of a step.  A Low-Delay-P deployment
 *      needs four models (model_LDP_200000_qp22 .. qp37) that differ only in the samples they keep (slot-0 QP) and in their seeds, and
 *      read the same sample file.  A step of the group is still 10 launches, each over all members (csrc/ethcnn_lstm_train.h "trainer
 *      group"); an evaluation is still launches 1-4 over pieces of max(batch, 256) samples, then one loss launch.
 *   Exactness: member m computes what ethcnn_lstm_train_* computes for a trainer with opts[m], its weights, its QP list and its own
 *      upload of the same bytes -- bit for bit, whatever k is and wherever in the group the member sits.  The members share the
 *      records and nothing else: each has its own weights, accumulators, RNG streams (opts[m].seed), batch-global label counts,
 *      global norm, clip and learning rate.
 *   Members of one group have the same batch; every other option may differ.  ethcnn_lstm_train_group_check (host only, no context)
 *      returns ETHCNN_ERR_ARG and a message that names the member and the field for differing batches and for an option
 *      ethcnn_lstm_train_create refuses; err may be NULL.
 *   Samples: ethcnn_lstm_train_group_set_qps(member) applies to the uploads that follow, as solo.  An upload keeps, per member, the
 *      list of the records whose slot-0 QP is in that member's list (file order; an empty list keeps all), and a member's sample
 *      index i means the i-th record it keeps -- what the solo trainer's index means -- so the index draw over its count gives the solo
 *      batches.  Only records at least one member keeps go to HBM and through the device validation: an upload returns
 *      ETHCNN_ERR_FORMAT exactly when some member's own solo upload would, with "member m: " in front of that member's solo message
 *      (the lowest such m), and ETHCNN_ERR_FORMAT with the member named when a member's selection is empty.  After a failed upload the
 *      group's previous set is still in place.  ethcnn_lstm_train_group_set_samples_from: take != 0 adopts the set's buffer whatever
 *      the members keep (the set is empty afterwards), else ONE device-to-device copy.
 *   Arrays over members are member-major: seeds[k], loss[k][3], acc[k][3], idx[k][n], probs[k][20 n][21].
 *   A member index outside 0..k-1 is ETHCNN_ERR_ARG. */
typedef struct ethcnn_lstm_train_group ethcnn_lstm_train_group;
int ethcnn_lstm_train_group_check(const ethcnn_lstm_train_options* opts, int k, char* err, size_t errcap);
/* host only: the records (indices, file order) of a sample file that a member with this QP list keeps; keep may be NULL (count only),
 * else it holds nbytes / 37264 entries.  ERR_FORMAT when nbytes is not a whole number of samples. */
int ethcnn_lstm_train_group_keep_list(const uint8_t* records, size_t nbytes, const int* qps, int nqps, int64_t* keep, int64_t* nkept);
int ethcnn_lstm_train_group_create(ethcnn_ctx* ctx, const ethcnn_lstm_train_options* opts, int k, ethcnn_lstm_train_group** out);
void ethcnn_lstm_train_group_destroy(ethcnn_lstm_train_group* grp); /* before ethcnn_destroy of its context */
int ethcnn_lstm_train_group_init_weights(ethcnn_lstm_train_group* grp, const uint64_t* seeds /* [k] */);
int ethcnn_lstm_train_group_set_blob(ethcnn_lstm_train_group* grp, int member, const float* blob, const float* accum /* NULL = zeros */, size_t nfloats);
int ethcnn_lstm_train_group_get_blob(ethcnn_lstm_train_group* grp, int member, float* blob, float* accum /* may be NULL */, size_t nfloats);
int ethcnn_lstm_train_group_set_qps(ethcnn_lstm_train_group* grp, int member, const int* qps, int nqps); /* applies to the uploads that follow */
int ethcnn_lstm_train_group_set_samples(ethcnn_lstm_train_group* grp, int set, const uint8_t* records, size_t nbytes);
int64_t ethcnn_lstm_train_group_num_samples(const ethcnn_lstm_train_group* grp, int member, int set); /* samples the member keeps */
/* steps first_step .. first_step + nsteps - 1 of every member, device-drawn batches; asynchronous (nothing read back) */
int ethcnn_lstm_train_group_run(ethcnn_lstm_train_group* grp, int64_t first_step, int64_t nsteps);
int ethcnn_lstm_train_group_last_stats(ethcnn_lstm_train_group* grp, float* loss /* [k][3] */, float* acc /* [k][3] */);
/* one step on explicit batches, n == batch samples per member: idx [k][n], each row in that member's own kept indices; synchronous */
int ethcnn_lstm_train_group_step_indices(ethcnn_lstm_train_group* grp, int64_t step, const int32_t* idx, int n, float* loss, float* acc);
/* forward only: member m over its samples idx[m][0..n-1] (its own kept indices), or, idx NULL, over its samples 0 .. n-1 (n must
 * then be <= every member's count); each member's loss and accuracy lists are those of ONE batch of all its n samples.
 * probs [k][20 n][21] may be NULL. */
int ethcnn_lstm_train_group_evaluate(ethcnn_lstm_train_group* grp, int set, const int32_t* idx, int64_t n, float* loss, float* acc, float* probs);
int ethcnn_lstm_train_group_debug_fetch(ethcnn_lstm_train_group* grp, int member, int which, float* out, size_t nfloats);
int64_t ethcnn_lstm_train_group_debug_rows(const ethcnn_lstm_train_group* grp, int member);
const char* ethcnn_lstm_train_group_last_error(const ethcnn_lstm_train_group* grp);

/* ---- sample sets (Extract_Data/extract_data_AI.py:94-170, extract_data_LDP_LDB_RA.py:68-208): the trainers' sample records cut out of
 *      YUV and label files into HBM, handed to a trainer there, or written as the reference's sample files, byte for byte.
 *   Samples are the WHOLE 64 x 64 CTUs of a frame, (height / 64) x (width / 64) of them in raster order (the ragged right and bottom
 *      edges are dropped, not padded); records follow in the order sequence (as added), frame, CTU.
 *   Label files (*_CUDepth.dat): one byte per 16 x 16 block, (height / 16) x (width / 16) per frame, raster, frames in file order.
 *   ETHCNN_SAMPLES_AI: the 4992-byte record of "training" above, every byte 255 except the luma at 0 and, for each QP q of the list,
 *      the CTU's 4 x 4 depth bytes (raster) at 4160 + 16 q.  One YUV per sequence, one label file per QP, every frame of the file.
 *   ETHCNN_SAMPLES_INTER (Low-Delay-P, Low-Delay-B, Random-Access): the 16516-byte record, every byte 255 except header byte 0 = 1,
 *      2-3 width, 4-5 height, 10-13 frame number in encoding order, 14-15 CTU line, 16-17 CTU column, 18-19 the sequence's position in
 *      the order of the add calls (little-endian), and slot s at 64 + 4113 s = [qps[s] | 16 depth bytes | 4096 residual bytes], the
 *      residual from the s-th residual file.  Four QPs, four residual YUVs and four label files per sequence.  Frames 1 .. n-1 in
 *      encoding order (the initial I-frame is skipped).  The frame READ from the files for frame i in encoding order is i itself
 *      (ETHCNN_SAMPLES_ORDER_ENCODE: LDP, LDB) or, ETHCNN_SAMPLES_ORDER_RA, 1 + T[(i - 1) % 8] + 8 g with g = (i - 1) / 8 and T =
 *      (7 3 1 0 2 5 4 6) without the entries >= min(n - 1 - 8 g, 8) -- the shortened table of a last GOP of fewer than 8 frames.
 *   The permutation (shuffled reads and files): record j of the output is record perm(j) of the set, with, for count records,
 *      h = the smallest integer >= 1 with 4^h >= count, mask = 2^h - 1, and draw() of "training" above on stream 7:
 *        x = j; repeat { l = x >> h; r = x & mask; for round = 0..3: (l, r) = (r, l ^ (draw(7, count, r, round) & mask)); x = l << h | r }
 *        until x < count; perm(j) = x
 *      (a four-round Feistel network over 2 h bits, cycle-walked into [0, count): a bijection fixed by (seed, count), computed per
 *      record; the reference's own shuffle is Python's unseeded random.sample and is not reproduced.)
 *   Source format (All-Intra sets): a sequence's YUV is read in the format in force when it is added, "high-bit-depth and non-4:2:0
 *      sources" above: planar, luma first, one byte per sample at bit depth 8 and an unsigned 16-bit little-endian container above,
 *      chroma planes of the size the chroma format demands (never read).  The luma a record holds is min(s >> (bit_depth - 8), 255),
 *      THE NARROWING RULE above, so a deep re-encoding s16 = s8 << (bit_depth - 8) | low bits of a file gives the 8-bit file's records
 *      byte for byte.  The default {8, 420} is the reference's only format.  Inter sets refuse every other format: HM's residual
 *      writer always emits 8-bit 4:2:0.
 *   A set belongs to a context (its device, stream and fill threads); ctx == NULL gives a set that validates and counts only. */
typedef struct ethcnn_samples ethcnn_samples;
enum { ETHCNN_SAMPLES_AI = 0, ETHCNN_SAMPLES_INTER = 1 };
enum { ETHCNN_SAMPLES_ORDER_ENCODE = 0, ETHCNN_SAMPLES_ORDER_RA = 1 };
/* qps: All-Intra 1..52 distinct QPs in 0..51; inter exactly four distinct, in slot order.  max_bytes: the largest set
 * ethcnn_samples_build may allocate, 0 = no limit of its own. */
int ethcnn_samples_create(ethcnn_ctx* ctx /* may be NULL */, int kind, const int* qps, int nqps, int frame_order, uint64_t max_bytes,
                          ethcnn_samples** out);
void ethcnn_samples_destroy(ethcnn_samples* set); /* before ethcnn_destroy of its context */
const char* ethcnn_samples_last_error(const ethcnn_samples* set);
/* The source format of the sequences added AFTER this call (sticky: one set may mix 8-bit and 10-bit sequences; default {8, 420}).
 * ETHCNN_ERR_ARG: an invalid format, anything but {8, 420} on an ETHCNN_SAMPLES_INTER set, a set that is built.  Works on a set
 * without a context. */
int ethcnn_samples_set_source_format(ethcnn_samples* set, const ethcnn_source_format* fmt);
/* Validates and counts, nothing more.  nyuv = 1 (All-Intra) or 4 (inter: the residual file of each slot), nlabels = the QP count, label
 * paths in QP-list order.  ETHCNN_ERR_FORMAT, with the file named: width or height below 64 or not a multiple of 8, a YUV that is not a
 * whole number of frames of the source format in force (ethcnn_source_frame_bytes; the message names the format unless it is 8-bit
 * 4:2:0), residual files of different frame counts, a label file whose size is not frames x (h / 16) x (w / 16).
 * ETHCNN_ERR_IO: a file that cannot be examined. */
int ethcnn_samples_add_sequence(ethcnn_samples* set, int width, int height, const char* const* yuv_paths, int nyuv,
                                const char* const* label_paths, int nlabels);
int64_t ethcnn_samples_count(const ethcnn_samples* set); /* records of the sequences added so far */
int ethcnn_samples_record_bytes(const ethcnn_samples* set);
/* One allocation of count x record_bytes in HBM (ETHCNN_ERR_NOMEM, with the byte count, when it does not fit or exceeds max_bytes;
 * nothing is allocated then), filled sequence by sequence, a bounded number of frames at a time: luma and label planes are read by the
 * context's fill threads into page-locked staging (chroma is never read), copied to HBM and cut into records by the kernel while the next
 * frames are read.  Luma above 8 bits is uploaded as it is in the file, two bytes per sample, and narrowed by the cut kernel (the
 * kernel of ethcnn_samples_cut16_device); 8-bit luma of any chroma format takes the kernel of ethcnn_samples_cut_device.
 * Synchronous.  Once; sequences cannot be added afterwards. */
int ethcnn_samples_build(ethcnn_samples* set);
/* The kernel alone, on frames already in HBM: `nframes` frames of d_luma[p] (p = 0, or the four slots; `pitch[p]` bytes between rows,
 * `frame_stride[p]` between frames) and of d_labels[q] (one per QP of the list, frames packed) become records record_offset .. of
 * d_records (16-byte aligned, inter: 4-byte), frame f with frame number frame_number + f (inter header).  Any alignment of the luma
 * pointers and pitches gives the same bytes (16-byte aligned ones take the wide loads).  Asynchronous on the context's stream. */
int ethcnn_samples_cut_device(ethcnn_ctx* ctx, int kind, const int* qps, int nqps, int width, int height, int nframes,
                              const uint8_t* const* d_luma, const ptrdiff_t* pitch, const ptrdiff_t* frame_stride,
                              const uint8_t* const* d_labels, int frame_number, int seq_number, uint8_t* d_records, int64_t record_offset);
/* The All-Intra cut over 16-bit luma: as ethcnn_samples_cut_device with kind ETHCNN_SAMPLES_AI, the frames being unsigned 16-bit
 * little-endian planes at d_luma16 (any 2-byte aligned address; pitch_bytes even and >= 2 width; frame_stride_bytes even) and the luma
 * of a record min(s >> (bit_depth - 8), 255), bit_depth 8..16.  One kernel: nothing is narrowed into memory first.  Every alignment
 * gives the same bytes (bases, pitches and strides that are multiples of 16 take the wide loads).  Only whole CTUs are read: nothing
 * outside rows [0, 64 (height / 64)) or columns [0, 64 (width / 64)) of a plane.  ETHCNN_ERR_ARG: a bit depth outside 8..16, an odd
 * address, pitch or stride, and whatever ethcnn_samples_cut_device refuses.  Asynchronous on the context's stream. */
int ethcnn_samples_cut16_device(ethcnn_ctx* ctx, const int* qps, int nqps, int width, int height, int nframes, const uint16_t* d_luma16,
                                ptrdiff_t pitch_bytes, ptrdiff_t frame_stride_bytes, int bit_depth, const uint8_t* const* d_labels,
                                uint8_t* d_records, int64_t record_offset);
/* records [first, first + n) of the built set (permuted != 0: of its permutation by `seed`) -> host memory */
int ethcnn_samples_read(ethcnn_samples* set, int64_t first, int64_t n, int permuted, uint64_t seed, uint8_t* out);
/* the whole set as a sample file (temp file + rename: never a partial file); permuted != 0: the "_shuffled" form */
int ethcnn_samples_write(ethcnn_samples* set, const char* path, int permuted, uint64_t seed);
/* A built set becomes set 0 / 1 of a trainer of the same context without leaving HBM.  ETHCNN_ERR_FORMAT when the kind does not match
 * the trainer's net; for the LDP net the slot-QP pass of ethcnn_train_set_samples runs on the device copy and the QP list defaults to
 * the four slots, as there.  take != 0: the trainer adopts the buffer and the set becomes empty (0 records, not built); else a
 * device-to-device copy. */
int ethcnn_train_set_samples_from(ethcnn_trainer* tr, int set_index, ethcnn_samples* set, int take);
/* the same for a trainer group ("training, several models at once"): one buffer serves every member */
int ethcnn_train_group_set_samples_from(ethcnn_train_group* grp, int set_index, ethcnn_samples* set, int take);

/* ---- ETH-LSTM sample sets (ETH-LSTM_Training_LDP/get_LSTM_input.py): the 37264-byte samples of "ETH-LSTM training" above, built in HBM
 *      from 16516-byte Low-Delay-P records (an inter sample set that is resident there, or records in host memory) with the context's
 *      residual CNN, handed to an LSTM trainer there, or written as the file get_LSTM_input.py writes, byte for byte.
 *   Definition.  For each requested QP slot in ascending slot order, for each record r in file order whose i_frame (little-endian u32 at
 *      info byte 10) is >= 19 and a multiple of 10: time slot k = 0..19 takes record r - k * (width / 64) * (height / 64) (integer
 *      divisions; width = u16 at info byte 2, height = u16 at byte 4, both of r's OWN header).  A head whose slot-19 reference is
 *      negative is skipped and counted.  No other check ties a reference to the head's sequence: a file that holds several sequences or
 *      geometries gives what this rule gives.  The sample is r's 64 info bytes with byte 0 set to 19, then for every k 465 float32:
 *      [QP byte | 16 label bytes | 448-vector] of the referenced record at that slot, the bytes converted to float, the vector what
 *      ethcnn_resi_vectors* gives for the slot's 4096 residual bytes (a 64 x 64 picture) with the CNN the context has loaded -- the
 *      same bits whichever picture shape and pass form compute it.  With m heads kept and the slots s_0 < s_1 < ..., sample
 *      i m + j is head j at slot s_i.  The order is fixed by this rule alone (no atomics, no scheduling).
 *   slots: the QP slots (0..3, distinct, any order) to build; nslots = 0: all four.  One LSTM model is trained per QP, so a caller who
 *      trains one QP builds one slot, at a quarter of the work and memory.
 *   chunk_ctus: records whose residuals go through the CNN per chunk; 0 = default (8192), else a multiple of 32 and at most the
 *      context's max_ctus_per_pass.  max_bytes: the most device memory a build may allocate (samples + working buffers), 0 = no limit
 *      of its own.
 *   Memory of a build over n records with m heads: m x nslots x 37264 bytes of samples; working buffers, freed when the build returns:
 *      one slot's vectors (n rounded up to 32, x 1792 bytes; reused by the next slot), one chunk's picture (4096 x the smaller of
 *      chunk_ctus and n rounded up to 32), the plan (16 m) and, for records from host memory, their copy in HBM (n x 16516, uploaded in
 *      pieces of 64 MB).  That sum is what max_bytes is held against and what ETHCNN_ERR_NOMEM reports, before any of it is allocated.
 *      Outside the sum: a build from a set first holds 8 n bytes of record headers in HBM for the selection, freed before the check.
 *   Errors: ETHCNN_ERR_NOWEIGHTS when the context has no CNN loaded; ETHCNN_ERR_FORMAT when nbytes is zero or not a whole number of
 *      16516-byte records, or the set is of kind ETHCNN_SAMPLES_AI or not built; ETHCNN_ERR_ARG for bad slots or a bad chunk_ctus;
 *      ETHCNN_ERR_NOMEM, with the byte count in the message, when the memory above exceeds max_bytes or does not fit -- nothing stays
 *      allocated then, and the object may build again.  A build on a built set replaces its samples.  All offsets are 64-bit. */
typedef struct ethcnn_lstm_samples ethcnn_lstm_samples;
/* The selection alone, on the host (no context, no GPU): heads[j] = record index of the j-th head kept, strides[j] = its
 * (width / 64) * (height / 64); both may be NULL, else they hold nbytes / 16516 entries.  ERR_FORMAT as above. */
int ethcnn_lstm_samples_plan(const uint8_t* records, size_t nbytes, int64_t* heads, int64_t* strides, int64_t* nheads, int64_t* skipped);
int ethcnn_lstm_samples_create(ethcnn_ctx* ctx, const int* slots, int nslots, int chunk_ctus, uint64_t max_bytes, ethcnn_lstm_samples** out);
void ethcnn_lstm_samples_destroy(ethcnn_lstm_samples* set); /* before ethcnn_destroy of its context */
const char* ethcnn_lstm_samples_last_error(const ethcnn_lstm_samples* set);
/* from a built inter set of the same context, which is only read and stays as it is */
int ethcnn_lstm_samples_build_from_set(ethcnn_lstm_samples* set, ethcnn_samples* inter_set);
int ethcnn_lstm_samples_build_from_records(ethcnn_lstm_samples* set, const uint8_t* records, size_t nbytes); /* host memory */
int64_t ethcnn_lstm_samples_count(const ethcnn_lstm_samples* set);   /* samples: heads kept x slots */
int64_t ethcnn_lstm_samples_skipped(const ethcnn_lstm_samples* set); /* heads skipped (counted once, not per slot) */
int ethcnn_lstm_samples_read(ethcnn_lstm_samples* set, int64_t first, int64_t n, uint8_t* out); /* samples [first, first + n) -> host */
int ethcnn_lstm_samples_write(ethcnn_lstm_samples* set, const char* path); /* temp file + rename: never a partial file */
/* A built set becomes set 0 / 1 of an LSTM trainer of the same context without leaving HBM, as if its bytes had gone through
 * ethcnn_lstm_train_set_samples: the QP list of an earlier ethcnn_lstm_train_set_qps selects on the slot-0 QP (kept samples in order)
 * and the same validation pass runs on the device.  When the selection keeps every sample and take != 0 the trainer adopts the buffer;
 * else it gets a device-to-device copy of the kept samples.  take != 0: the set is empty afterwards (0 samples, not built). */
int ethcnn_lstm_train_set_samples_from(ethcnn_lstm_trainer* tr, int set_index, ethcnn_lstm_samples* set, int take);
/* the same for an LSTM trainer group ("ETH-LSTM training, several models at once"): one buffer serves every member, each through
 * its own keep list; take != 0 always adopts the buffer */
int ethcnn_lstm_train_group_set_samples_from(ethcnn_lstm_train_group* grp, int set_index, ethcnn_lstm_samples* set, int take);
/* MEASUREMENT ENTRIES, not part of the feature's interface: they exist for scripts/lstm_samples_rate.py, may change or go without
 * notice, and nothing should be built on them.  All asynchronous on the context's stream.
 * repack / gather: the two kernels alone, on buffers already in HBM.  repack: the residuals of records first .. first + n - 1 (of
 * d_records' nrecords, 16-byte aligned) at `slot` -> d_picture, 2048 bytes a row, 64 rows per 32 records, record first + j at row
 * 64 (j / 32), column 64 (j % 32), the rest of the last 32 zero: the picture ethcnn_resi_vectors_device takes.  gather: sample j of
 * d_samples from head d_heads[j] with stride d_strides[j] (the caller's duty: every reference within 0 .. nrecords - 1) and the
 * vectors d_vectors [nrecords][448] of that slot.
 * copy: a float4 grid-stride copy (addresses and nbytes multiples of 16), the rate the byte-moving kernels are judged against. */
int ethcnn_bench_lstm_repack(ethcnn_ctx* ctx, const uint8_t* d_records, int64_t nrecords, int64_t first, int n, int slot, uint8_t* d_picture);
int ethcnn_bench_lstm_gather(ethcnn_ctx* ctx, const uint8_t* d_records, int64_t nrecords, const float* d_vectors, const int64_t* d_heads,
                             const int64_t* d_strides, int64_t nheads, int slot, uint8_t* d_samples);
int ethcnn_bench_copy(ethcnn_ctx* ctx, const void* d_src, void* d_dst, size_t nbytes);

/* ---- threshold calibration: Thr_info.txt from labelled predictions (no reference counterpart: the reference ships hand-set values,
 *      0.5 x 6 for All-Intra and 0.4 0.6 0.3 0.7 0.2 0.8 for LDP).  HM takes "split only" when p > up[depth] and "current only" when
 *      p <= down[depth] and runs the full rate-distortion search in between (HM-16.5_Test_AI/.../TEncCu.cpp:448-455).  A calibrator
 *      counts, on the GPU, where the probabilities of truly split and truly unsplit samples fall; the choice and the file are host work.
 *   Truth and populations (tools/score_cu_depth.py:47-65 in integers).  A CTU carries 16 depth bytes d[0..15] (0..3, the 4 x 4 raster of
 *      its 16 x 16 blocks) and 21 probabilities p[0..20]; IDX32 = {{0,1,4,5},{2,3,6,7},{8,9,12,13},{10,11,14,15}}.
 *        level 0: every CTU,                                          probability p[0],               split when t64 = (sum d > 8)
 *        level 1: each 32 x 32 block j of a CTU with t64,              probability p[1 + j],           split when t32[j] = (sum_i d[IDX32[j][i]] > 6)
 *        level 2: each 16 x 16 block i of a block j with t64 and t32[j], probability p[5 + IDX32[j][i]], split when d[IDX32[j][i]] == 3
 *   Bins: 1025 per (level, truth).  bin(p) = ceil(p * 1024) in fp32 (the product is exact): bin 0 holds p == 0, bin j >= 1 holds
 *      (j - 1) / 1024 < p <= j / 1024.  So HM's comparisons are exact on the grid t_k = k / 1024: p > t_k <=> bin > k, p <= t_k <=> bin <= k.
 *      A probability that is NaN, below 0 or above 1 is counted in rejected[level] and binned nowhere.  A depth byte above 3 fails the
 *      call with ETHCNN_ERR_FORMAT (the kernel raises a flag word that the host reads; nothing faults) and the call adds NOTHING.
 *   Accumulator: hist[3][2][1025] (level, truth, bin) and rejected[3], uint64; over frame layouts also skipped_partial.  Counts are exact
 *      integers and do not depend on the grid, on the order of calls or on how a set is split over calls.
 *   Layouts.  Per-CTU: probs float32 [n][21], depth16 uint8 [n][16] (a training sample's label bytes).  Frame: labels uint8
 *      [skip_label_frames + nframes][height / 16][width / 16] (an Info_*_CUDepth.dat; width and height multiples of 16, else
 *      ETHCNN_ERR_ARG), of which the first skip_label_frames frames are passed over (tools/score_cu_depth.py --skip-label-frames: LDP
 *      predictions start at POC 1); probs float32 [nframes][ceil(height / 64) * ceil(width / 64)][21].  The kernel gathers each CTU's
 *      4 x 4 map itself.  A CTU that is not wholly inside the picture is left out and counted in skipped_partial: HM forces those
 *      splits and they have no full label map.
 *   Gates: the predictors' batch gates zero whole sub-batches of p32 / p16, so the probabilities must have been predicted with open
 *      gates, ethcnn_set_thresholds(ctx, 0, 0).  The calibrator cannot see how a buffer it is given was made.
 *   Every add entry is synchronous (it waits for the flag word); device pointers must be 4-byte aligned.  n == 0 / nframes == 0: no-op.
 *   Errors: the usual codes, text in ethcnn_last_error of the calibrator's context (of NULL for the two context-free entries). */
typedef struct ethcnn_calib ethcnn_calib;
#define ETHCNN_CALIB_BINS 1025
#define ETHCNN_CALIB_HIST_WORDS (3 * 2 * ETHCNN_CALIB_BINS)
int ethcnn_calib_create(ethcnn_ctx* ctx, ethcnn_calib** out);
void ethcnn_calib_destroy(ethcnn_calib* cal); /* before ethcnn_destroy of its context */
int ethcnn_calib_reset(ethcnn_calib* cal);
int ethcnn_calib_add(ethcnn_calib* cal, const float* probs, const uint8_t* depth16, int64_t n); /* host pointers, staged in pieces */
int ethcnn_calib_add_device(ethcnn_calib* cal, const float* d_probs, const uint8_t* d_depth16, int64_t n);
int ethcnn_calib_add_frames(ethcnn_calib* cal, const float* probs, const uint8_t* labels, int width, int height, int64_t nframes,
                            int64_t skip_label_frames);
int ethcnn_calib_add_frames_device(ethcnn_calib* cal, const float* d_probs, const uint8_t* d_labels, int width, int height,
                                   int64_t nframes, int64_t skip_label_frames);
/* waits for the stream; every pointer may be NULL.  hist: ETHCNN_CALIB_HIST_WORDS words */
int ethcnn_calib_get(ethcnn_calib* cal, uint64_t* hist, uint64_t rejected[3], uint64_t* skipped_partial);
/* The choice (pure host, no context).  Budgets in parts per million.  Per level, with N1 / N0 the split / non-split totals,
 *      miss(k) = sum_{bin <= k} hist[l][1] (truly split, forced to "current only") and fsplit(k) = sum_{bin > k} hist[l][0]:
 *        down_k = the largest k in -1..1024 with miss(k) * 10^6 <= eps_down_ppm * N1   (-1 always qualifies: "never current only")
 *        up_k   = the smallest k in 0..1024 with fsplit(k) * 10^6 <= eps_up_ppm * N0   (1024 always qualifies: "never split only")
 *      (128-bit products).  When down_k > up_k both become the k in [up_k, down_k] with the least miss(k) + fsplit(k), the lowest at
 *      ties; every k of that range meets both budgets.  Budgets above 10^6 are ETHCNN_ERR_ARG. */
typedef struct ethcnn_calib_level {
    uint64_t n0, n1;         /* non-split / split samples of the level                                      */
    int32_t down_k, up_k;    /* the thresholds are down_k / 1024 and up_k / 1024                            */
    double down, up;
    uint64_t miss, fsplit;   /* miss(down_k), fsplit(up_k)                                                  */
    uint64_t uncertain;      /* samples of either truth with down_k < bin <= up_k: the full search remains  */
    double uncertain_share;  /* uncertain / (n0 + n1); 0 for a level without samples                        */
    double accuracy_512;     /* accuracy of the plain decision p > 0.5; 0 for a level without samples       */
    int32_t empty_class;     /* n0 == 0 or n1 == 0: the budgets constrain nothing on that side              */
    int32_t crossed;         /* down_k > up_k before the joint choice                                       */
} ethcnn_calib_level;
typedef struct ethcnn_calib_report {
    ethcnn_calib_level level[3];
} ethcnn_calib_report;
int ethcnn_calib_choose(const uint64_t* hist, const uint32_t eps_down_ppm[3], const uint32_t eps_up_ppm[3], ethcnn_calib_report* report);
/* One line of six values k / 1024 with 10 decimals (every k / 1024 has at most 10, so fscanf("%f") and float() read it back exactly),
 * temp file + rename.  THE TWO ENCODERS DIFFER in token order:
 *   ETHCNN_THR_ORDER_AI   up1 down1 up2 down2 up3 down3   (HM-16.5_Test_AI/source/Lib/TLibEncoder/TEncCu.cpp:250)
 *   ETHCNN_THR_ORDER_LDP  down1 up1 down2 up2 down3 up3   (HM-16.5_Test_LDP/source/Lib/TLibEncoder/TEncGOP.cpp:1449)
 * The predictors (ethcnn_load_thresholds) read tokens [1] and [3] of either file, as the reference's do. */
enum { ETHCNN_THR_ORDER_AI = 0, ETHCNN_THR_ORDER_LDP = 1 };
int ethcnn_calib_write_thr_info(const char* path, const ethcnn_calib_report* report, int order);

/* ---- partition-search simulation: what HM's pruned CU search does under a candidate Thr_info.txt (no reference counterpart).  The
 *      calibrator above counts teacher-forced populations and knows no cost; a simulator evaluates HM's three-way rule
 *      (HM-16.5_Test_AI/source/Lib/TLibEncoder/TEncCu.cpp:419-463; HM-16.5_Test_LDP/.../TEncCu.cpp:421-470 is identical) over every
 *      CTU of a set that stays in HBM, for any number of candidate files at once, and counts the rate-distortion (RD) checks that
 *      remain and, with labels, the labelled partitions the pruned search can no longer reach.
 *   The rule.  A CU of size s = 64 >> depth has its top-left luma sample at (x, y) of a W x H picture (W, H multiples of 8, as HM
 *      requires; else ETHCNN_ERR_ARG).  A CTU's 64 x 64 CU is visited; a visited CU is treated by the first line that applies:
 *        1. x >= W or y >= H: not visited at all (HM's own sub-CU loop).
 *        2. s == 8: checked, no recursion.  checked[3] += 1.
 *        3. x + s > W or y + s > H (the frame edge): nothing is checked, its four sub-CUs are visited.  edge_split[depth] += 1.
 *           (HM writes uiRPelX >= iWidth || uiBPelY > iHeight with uiRPelX = x + s - 1; for W, H multiples of 8 the > and >= forms
 *           coincide.)
 *        4. else a DECIDED NODE with probability p[0] (64), p[1 + x32 + 2 y32] (32) or p[5 + x16 + 4 y16] (16), x32 .. y16 the block
 *           coordinates inside the CTU, and bin = ceil(p * 1024) in fp32 exactly as in the calibration block.  A candidate is six
 *           integers on that grid, up_k[3] in 0..1024 and down_k[3] in -1..1024 (else ETHCNN_ERR_ARG); with d = depth, in HM's order:
 *             bin > up_k[d]         SPLIT ONLY    nothing is checked, the four sub-CUs are visited   split_only[d] += 1
 *             else bin <= down_k[d] CURRENT ONLY  the CU is checked, no recursion                    current_only[d] += 1, checked[d] += 1
 *             else                  BOTH          the CU is checked, the four sub-CUs are visited    both[d] += 1, checked[d] += 1
 *           down_k > up_k is allowed: the order of the tests decides.
 *      up_k = 1024, down_k = -1 on all levels is the full search: every node lands in BOTH.
 *   Gates.  The predictors zero whole sub-batches of p32 / p16 (<= 1024 consecutive CTUs of one frame), so in the frame layouts each
 *      sub-batch carries M1 = max bin(p[0]) and M2 = max bin(p[1..4]) over its CTUs' probabilities as given.  With gate thresholds
 *      g1, g2:  gate 1 is open <=> M1 > g1;  gate 2 is open <=> (gate 1 open ? M2 : 0) > g2;  a closed gate 1 makes every p32 bin of
 *      the sub-batch 0, a closed gate 2 every p16 bin (bin 0 against down_k = -1 lands in BOTH: the "0 > thr2" corner).  gate_order:
 *        ETHCNN_SIM_GATES_NONE  no gates: the probabilities are what the encoder will read
 *        ETHCNN_SIM_GATES_AI    g1 = down_k[0], g2 = down_k[1]  (tokens [1], [3] of an AI-order file; while down_k <= up_k on levels 0
 *                                                                and 1 these gates change no decision)
 *        ETHCNN_SIM_GATES_LDP   g1 = up_k[0],   g2 = up_k[1]    (tokens [1], [3] of an LDP-order file; these do change decisions, as
 *                                                                the reference's predictor does under such a file)
 *      CTUs added in the per-CTU layout belong to no sub-batch and are never gated.  For the gated orders the probabilities must have
 *      been predicted with open gates, as for the calibrator.
 *   Truth.  Labels are optional (NULL) in every add entry and are used on CTUs wholly inside the picture only; with labels, width and
 *      height must be multiples of 16 (else ETHCNN_ERR_ARG).  A depth byte above 3 fails the call with ETHCNN_ERR_FORMAT and the call
 *      adds NOTHING.  Flags as in the calibration block: node 64 is split when sum d > 8, node 32 j when sum_i d[IDX32[j][i]] > 6, node
 *      16 when d == 3.  Every decided node of a labelled CTU is judged by its own flag, whatever happened above it:
 *        wrong_split[d]  SPLIT ONLY on a node whose flag is unsplit      wrong_stop[d]  CURRENT ONLY on a node whose flag is split
 *        bad_ctus        labelled CTUs with at least one wrong node: if the full search would return the labelled partition, the
 *                        pruned search can no longer reach it
 *   A CTU with a NaN, a negative or a > 1 value among its 21 probabilities is left out of everything (counters, M1 / M2, labels) and
 *      counted in rejected_ctus.
 *   Everything is integers; counters are uint64 and do not depend on the grid, on the order of add calls or on how a set is split
 *      over calls.  The set costs 64 bytes per CTU of device memory (+ 8 per sub-batch); when it cannot grow the add fails with
 *      ETHCNN_ERR_NOMEM (the byte count is in the message) and changes nothing.
 *   Layouts: as for the calibrator (per-CTU: probs [n][21], depth16 [n][16] or NULL; frame: probs [nframes][ceil(H / 64) *
 *      ceil(W / 64)][21], labels [skip_label_frames + nframes][H / 16][W / 16] or NULL).  Every entry is synchronous on the context's
 *      stream; device pointers must be 4-byte aligned; n == 0 / nframes == 0 is a no-op. */
typedef struct ethcnn_sim ethcnn_sim;
enum { ETHCNN_SIM_GATES_NONE = 0, ETHCNN_SIM_GATES_AI = 1, ETHCNN_SIM_GATES_LDP = 2 };
typedef struct ethcnn_sim_thr {
    int32_t up_k[3];   /* 0..1024  */
    int32_t down_k[3]; /* -1..1024 */
} ethcnn_sim_thr;
typedef struct ethcnn_sim_counts {
    uint64_t checked[4];      /* CUs of 64, 32, 16, 8 that are RD-checked */
    uint64_t split_only[3], current_only[3], both[3]; /* decided nodes by outcome */
    uint64_t edge_split[3];   /* visited CUs that cross the frame edge */
    uint64_t wrong_split[3], wrong_stop[3], bad_ctus; /* labelled CTUs only */
} ethcnn_sim_counts;
typedef struct ethcnn_sim_set_info { /* all independent of the candidate */
    uint64_t ctus;          /* CTUs added, the rejected ones included */
    uint64_t whole_ctus;    /* not rejected and wholly inside the picture */
    uint64_t labelled_ctus; /* of those, with labels */
    uint64_t rejected_ctus;
    uint64_t sub_batches;
} ethcnn_sim_set_info;
int ethcnn_sim_create(ethcnn_ctx* ctx, ethcnn_sim** out);
void ethcnn_sim_destroy(ethcnn_sim* sim); /* before ethcnn_destroy of its context */
int ethcnn_sim_reset(ethcnn_sim* sim);    /* empties the set; its device memory is kept */
int ethcnn_sim_add(ethcnn_sim* sim, const float* probs, const uint8_t* depth16, int64_t n); /* host pointers, staged in pieces */
int ethcnn_sim_add_device(ethcnn_sim* sim, const float* d_probs, const uint8_t* d_depth16, int64_t n);
int ethcnn_sim_add_frames(ethcnn_sim* sim, const float* probs, const uint8_t* labels, int width, int height, int64_t nframes,
                          int64_t skip_label_frames);
int ethcnn_sim_add_frames_device(ethcnn_sim* sim, const float* d_probs, const uint8_t* d_labels, int width, int height, int64_t nframes,
                                 int64_t skip_label_frames);
int ethcnn_sim_info(ethcnn_sim* sim, ethcnn_sim_set_info* info);
/* out[c] = the counters of candidate cand[c] over the whole set; ncand == 0 is a no-op, an empty set gives zeroed output */
int ethcnn_sim_eval(ethcnn_sim* sim, const ethcnn_sim_thr* cand, int64_t ncand, int gate_order, ethcnn_sim_counts* out);
/* One eval over every value of one coordinate, the other five as in base.  coord 0..5 = down0, up0, down1, up1, down2, up2;
 * out[i] is the value -1 + i of a down (ETHCNN_SIM_SWEEP_MAX = 1026 entries) or i of an up (1025 entries). */
#define ETHCNN_SIM_SWEEP_MAX 1026
int ethcnn_sim_sweep(ethcnn_sim* sim, const ethcnn_sim_thr* base, int coord, int gate_order, ethcnn_sim_counts* out);
/* Coordinate descent made of sweeps.  cost = sum_d weight[d] * checked[d]; a candidate is feasible <=> bad_ctus * 10^6 <=
 * max_bad_ppm * labelled_ctus (128-bit products, as in ethcnn_calib_choose).  A round sweeps the coordinates in the order above and
 * sets each to its feasible value of least cost, the smallest k at ties; the search stops after a round that changes nothing or after
 * max_rounds rounds (rounds_out = rounds run, 0 allowed).  start infeasible, no labelled CTU, max_bad_ppm > 10^6 or max_rounds < 0:
 * ETHCNN_ERR_ARG.  The full search is always feasible, and its cost is the denominator of every "share of the full search".
 * counts_out / rounds_out may be NULL. */
int ethcnn_sim_search(ethcnn_sim* sim, const ethcnn_sim_thr* start, int gate_order, const uint64_t weight[4], uint32_t max_bad_ppm,
                      int max_rounds, ethcnn_sim_thr* thr_out, ethcnn_sim_counts* counts_out, int* rounds_out);
/* the line and token orders of ethcnn_calib_write_thr_info, from six grid values (host only, no context) */
int ethcnn_sim_write_thr_info(const char* path, const ethcnn_sim_thr* thr, int order);

/* ---- partition decisions: the rule of "partition-search simulation" above under ONE candidate, written out per node of every CTU of a
 *      simulator's set instead of summed (no reference counterpart).  Where the simulator answers "how many checks remain", this
 *      answers "where": which nodes are checked, split or forced against their label, which depths stay reachable per 16 x 16 block,
 *      and the one partition the predictor prefers, in the label format of Info_*_CUDepth.dat.
 *   Input: CTUs first .. first + n of the set of `sim` (set order = the order of the add calls), the candidate thr (the simulator's
 *      ranges, else ETHCNN_ERR_ARG), gate_order as for ethcnn_sim_eval -- the gates are applied exactly as there: a closed gate makes
 *      the level's bins 0 BEFORE the rule and before the comparison with mid_k -- and mid_k in 0..1024 (else ETHCNN_ERR_ARG), on the same
 *      k / 1024 grid.  first < 0, n < 0 or first + n above the set's size: ETHCNN_ERR_ARG.
 *   Outputs, per CTU; nodes and blocks in the RASTER order of the 21 probabilities (node 0 = 64 x 64, 1 + x32 + 2 y32, 5 + x16 + 4 y16;
 *      block b = x16 + 4 y16), whatever order the set keeps inside:
 *      codes  uint8 [n][24]
 *        bytes 0..20  one code per node: 0 not visited (rule 1 included), 1 CURRENT ONLY, 2 SPLIT ONLY, 3 BOTH, 4 split because the CU
 *                     crosses the frame edge (rule 3); 8 is OR-ed in where a labelled CTU is forced against its label: 2 | 8 is a
 *                     wrong_split, 1 | 8 a wrong_stop of the simulator's counters
 *        byte 21      flags: bit 0 bad CTU (some node carries the 8), bit 1 labelled, bit 2 rejected, bit 3 the level-1 gate of the CTU's
 *                     sub-batch is closed, bit 4 the level-2 gate is closed (a closed level-1 gate reads M2 as 0, as in the simulator)
 *        byte 22      the 8 x 8 CUs that are checked, 0..64 (rule 2: four under a 16 x 16 node with code 2 or 3, the two or the one inside
 *                     the picture under one with code 4)
 *        byte 23      0
 *        A rejected CTU has codes 0, flags 4 (bit 2 alone) and byte 22 = 0.
 *      reach  uint8 [n][16]: bit d (0..3) of block b is set <=> the pruned search can still give block b depth d: every node above
 *        depth d on b's path has code 2, 3 or 4 and the node at depth d has code 1 or 3; for d = 3 the 16 x 16 node has code 2, 3 or 4.
 *        (The 8 does not count.)  Blocks that start outside the picture and rejected CTUs get 0.
 *      depth  uint8 [n][16]: the ONE partition the predictor prefers, as depths 0..3: from the 64 x 64 node down, a node with code 2 or 4
 *        splits, with code 1 stops, with code 3 splits <=> its bin > mid_k (the strict > of HM's p > up; 512 is p > 0.5); a block's depth
 *        is the level of the node that stops above it, 3 when its 16 x 16 node splits.  Blocks that start outside the picture and
 *        rejected CTUs get 255.  depth always lies inside reach: bit depth[b] of reach[b] is set wherever depth[b] != 255.
 *        What the bad flag is NOT: a labelled CTU whose reach lacks its label's bit somewhere is bad, but a bad CTU need not lack one:
 *        the simulator judges every decided node by its own flag, "whatever happened above it", so a SPLIT ONLY node BELOW the label's
 *        leaf (reached through a BOTH node that the label does not split) is a wrong_split although the label stays reachable.
 *      planes uint8 [nframes][H / 16][W / 16] (frame form only): depth scattered into label planes, the layout of Info_*_CUDepth.dat.
 *        Every block inside the picture is written, those of partial CTUs included; nothing outside the planes is.
 *   counts_from_codes gives back the simulator's counters of any slice of codes: codes of ethcnn_decide* summed over the whole set EQUAL
 *      ethcnn_sim_eval of the same candidate and gate order in every field; slices by frame or sequence give the breakdowns.
 *   Any output pointer may be NULL (nothing of it is computed); device pointers must be 4-byte aligned (else ETHCNN_ERR_ARG); every
 *      entry is synchronous on the context's stream; n == 0 / nframes == 0 is a no-op; a call that fails leaves the outputs untouched.
 *      Every output byte has one writer and everything is integers: the bytes do not depend on the grid or on how a set is split. */
int ethcnn_decide_device(ethcnn_sim* sim, const ethcnn_sim_thr* thr, int gate_order, int mid_k, int64_t first, int64_t n, uint8_t* d_codes,
                         uint8_t* d_reach, uint8_t* d_depth);
/* The same into host memory, staged in pieces of ethcnn_decide_set_piece CTUs (0 = the default, 2^20) through one device buffer of
 * piece * (24 + 16 + 16) bytes (the outputs asked for only).  That size is checked against the free device memory before anything is
 * allocated: on shortage ETHCNN_ERR_NOMEM, the byte count in the message.  The bytes do not depend on the piece size. */
int ethcnn_decide(ethcnn_sim* sim, const ethcnn_sim_thr* thr, int gate_order, int mid_k, int64_t first, int64_t n, uint8_t* codes, uint8_t* reach,
                  uint8_t* depth);
int ethcnn_decide_set_piece(ethcnn_sim* sim, int64_t ctus);
/* The frame form: nframes whole frames from CTU `first` on, which must have been added as width x height frames by ethcnn_sim_add_frames*
 * (or ethcnn_replay_feed_sim): first on a frame boundary of such an add and all nframes inside it (adds of one geometry that follow
 * each other count as one), else ETHCNN_ERR_ARG.  d_codes [nframes * nctu][24], d_reach [nframes * nctu][16] as above; d_planes
 * [nframes][height / 16][width / 16] needs width and height to be multiples of 16 (else ETHCNN_ERR_ARG) and no alignment. */
int ethcnn_decide_frames_device(ethcnn_sim* sim, const ethcnn_sim_thr* thr, int gate_order, int mid_k, int64_t first, int width, int height,
                                int64_t nframes, uint8_t* d_codes, uint8_t* d_reach, uint8_t* d_planes);
/* Host only, no context: the ethcnn_sim_counts of codes [n][24]: checked[0..2] from codes 1 and 3, checked[3] from byte 22, split_only /
 * current_only / both / edge_split from codes 2 / 1 / 3 / 4, wrong_split / wrong_stop from the 8, bad_ctus from flag bit 0.  n == 0 gives
 * zeroes.  NULL or n < 0: ETHCNN_ERR_ARG; a byte that no ethcnn_decide* call writes: ETHCNN_ERR_FORMAT; both leave counts_out untouched. */
int ethcnn_decide_counts_from_codes(const uint8_t* codes, int64_t n, ethcnn_sim_counts* counts_out);

/* ---- search budget: a stated share of the full search held FRAME BY FRAME by an encoder that does not change (no reference
 *      counterpart).  HM reads Thr_info.txt once (HM-16.5_Test_AI/source/Lib/TLibEncoder/TEncCu.cpp:245-255: the file handles are
 *      static and later fscanfs hit the end of the file), so one file sets an average over a sequence and nothing per frame.  But HM's
 *      rule (TEncCu.cpp:448-462) only compares p with up and down: a cu_depth.dat whose values are 1.0 where a node is to be SPLIT ONLY,
 *      0.0 where CURRENT ONLY and 0.5 where BOTH, read under the fixed COMPANION file up = 0.75, down = 0.25, makes the unchanged encoder
 *      carry out any per-frame, per-node decision.  These entries count, per frame of a simulator's set, the checks that every rung of
 *      a LADDER of candidates leaves, pick one rung per frame under a budget, and bake the picked decisions into 21 floats per CTU.
 *   Ladder: K candidates (ethcnn_sim_thr[K], 1 <= K <= ETHCNN_BUDGET_MAX_RUNGS, each in the simulator's ranges, else ETHCNN_ERR_ARG); rung
 *      0 is meant to be the most thorough.  ethcnn_budget_default_ladder fills ETHCNN_BUDGET_DEFAULT_RUNGS = 513 rungs: rung j has
 *      up_k = 1024 - j and down_k = j - 1 on all three levels, so rung 0 is the full search and rung 512 leaves only bin == 512 to BOTH.
 *      The cost does not rise along that ladder (up falls and down rises with j); the choice below does not rely on it.
 *   Cost.  The gates are always ETHCNN_SIM_GATES_NONE: the baked file is what the encoder reads.  checked[f][k][0..3] are the
 *      simulator's checked[0..3] (ethcnn_sim_counts) over the CTUs of frame f of the window under rung k; rejected CTUs count nowhere.
 *      Column K is the full search (up_k = 1024, down_k = -1).  Layout uint32 [nframes][K + 1][4]; a frame has fewer than 2^24 CTUs
 *      (else ETHCNN_ERR_ARG), so 32 bits hold every counter.  cost = sum_d weight[d] * checked[d]; weight[d] < 2^32 (else ETHCNN_ERR_ARG),
 *      default 64 16 4 1 as everywhere.  Integers only: the counters do not depend on the grid or on how a frame is cut over waves.
 *   Choice (ethcnn_budget_choose: host only, pure, no context).  Per frame f in order, with full_f = cost[f][K], in units of cost x 10^6
 *      and 128-bit products as in ethcnn_calib_choose:
 *        allow_f = budget_ppm * full_f + carry_{f-1}                      (carry_{-1} = 0: it starts at the first frame of the call)
 *        rung_f  = the smallest k in 0..K-1 with cost[f][k] * 10^6 <= allow_f
 *        no such k: rung_f = the rung of least cost (the smallest k at ties), over[f] = 1 and carry_f = 0
 *        ETHCNN_BUDGET_FRAME: carry_f = 0 always.   ETHCNN_BUDGET_CARRY: carry_f = allow_f - cost[f][rung_f] * 10^6.
 *      Outputs per frame: rung (int32), over (uint8, 0 / 1), cost = cost[f][rung_f] and full = full_f (uint64); each may be NULL.
 *      budget_ppm > 10^6, K outside 1..4096, an unknown mode, NULL checked (with nframes > 0) or weight, nframes < 0, a weight of 2^32
 *      or more, or a cost that does not fit in 64 bits (no frame below 2^24 CTUs gives one): ETHCNN_ERR_ARG, outputs untouched.
 *   Companion thresholds: ethcnn_budget_companion_thr gives up_k = 768, down_k = 256 on all levels; ethcnn_sim_write_thr_info writes them
 *      in either token order ("0.75 0.25 0.75 0.25 0.75 0.25" for All-Intra).  The encoder must read THAT file beside a baked cu_depth.dat.
 *   Baked values: one row of 21 float32 per CTU in the RASTER order of the 21 probabilities, by the codes of "partition decisions" under
 *      the rung of the CTU's frame, gates none:
 *        SPLIT ONLY (2) 1.0f     CURRENT ONLY (1) 0.0f     BOTH (3) 0.5f     frame-edge node (4, rule 3) 1.0f     not visited (0) 0.0f
 *        every node of a REJECTED CTU 0.5f: it gets the full search.
 *      Under the companion thresholds 1.0 is bin 1024 > 768, 0.0 is bin 0 <= 256 and 0.5 is bin 512 in between: ethcnn_decide* over the
 *      baked rows, gates none, gives every non-rejected CTU the codes bytes 0..22 it has on the original set under its frame's rung.  The
 *      three values are constants: no float arithmetic, every float has one writer, and the bytes do not depend on the grid or the pieces.
 *   Windows are those of ethcnn_decide_frames_device: nframes whole frames from CTU `first` on, inside one run of width x height frames,
 *      `first` on a frame boundary of it (else ETHCNN_ERR_ARG).  Every entry is synchronous on the context's stream; device pointers must
 *      be 4-byte aligned (else ETHCNN_ERR_ARG); nframes == 0 is a no-op; a call that fails leaves its outputs untouched. */
#define ETHCNN_BUDGET_DEFAULT_RUNGS 513
#define ETHCNN_BUDGET_MAX_RUNGS 4096
enum { ETHCNN_BUDGET_FRAME = 0, ETHCNN_BUDGET_CARRY = 1 };
int ethcnn_budget_default_ladder(ethcnn_sim_thr* out /* [ETHCNN_BUDGET_DEFAULT_RUNGS] */); /* host only, no context */
int ethcnn_budget_companion_thr(ethcnn_sim_thr* out);                                      /* host only, no context */
int ethcnn_budget_choose(const uint32_t* checked, int64_t nframes, int64_t K, const uint64_t weight[4], uint32_t budget_ppm, int mode,
                         int32_t* rung_out, uint8_t* over_out, uint64_t* cost_out, uint64_t* full_out);
/* checked_out uint32 [nframes][K + 1][4] in host memory / in HBM */
int ethcnn_budget_cost(ethcnn_sim* sim, const ethcnn_sim_thr* ladder, int64_t K, int64_t first, int width, int height, int64_t nframes,
                       uint32_t* checked_out);
int ethcnn_budget_cost_device(ethcnn_sim* sim, const ethcnn_sim_thr* ladder, int64_t K, int64_t first, int width, int height, int64_t nframes,
                              uint32_t* d_checked_out);
/* rung int32 [nframes] in HOST memory, each in 0..K-1 (else ETHCNN_ERR_ARG); probs float32 [nframes * nctu][21] in HBM / in host memory.
 * The host form is staged in pieces of ethcnn_decide_set_piece CTUs (0 = the default, 2^20; a piece may start inside a frame) through one
 * device buffer of piece * 84 bytes, checked against the free device memory first (ETHCNN_ERR_NOMEM); the bytes do not depend on it. */
int ethcnn_budget_bake_device(ethcnn_sim* sim, const ethcnn_sim_thr* ladder, int64_t K, const int32_t* rung, int64_t first, int width, int height,
                              int64_t nframes, float* d_probs_out);
int ethcnn_budget_bake(ethcnn_sim* sim, const ethcnn_sim_thr* ladder, int64_t K, const int32_t* rung, int64_t first, int width, int height,
                       int64_t nframes, float* probs_out);
/* cost, then choose, then bake in one call, into host memory.  ladder NULL: the default ladder (K is not read); weight NULL: 64 16 4 1.
 * probs_out [nframes * nctu][21] and the four per-frame outputs of ethcnn_budget_choose; any of them may be NULL (a NULL probs_out
 * skips the bake). */
int ethcnn_budget_control(ethcnn_sim* sim, const ethcnn_sim_thr* ladder, int64_t K, const uint64_t weight[4], uint32_t budget_ppm, int mode,
                          int64_t first, int width, int height, int64_t nframes, float* probs_out, int32_t* rung_out, uint8_t* over_out,
                          uint64_t* cost_out, uint64_t* full_out);

/* ---- search budget, online: the budget above held ONE FRAME AT A TIME, for a loop that has no sequence to pre-process (the Low-Delay-P
 *      daemons: the encoder produces one residual frame and blocks on its prediction).  A PACER owns what carries over from frame to
 *      frame -- the ladder, the weights, the budget, the mode, the 128-bit carry and the frame count -- and turns one frame's
 *      probabilities into its baked rows in two launches on the context's stream: one kernel packs the frame's records, counts the checks
 *      of every rung and makes the choice ON THE DEVICE, the bake kernel of "search budget" writes the rows.  No reference counterpart.
 *   Argument rules: ladder, K, weights, budget_ppm, mode and the W / H rule are exactly those of "search budget" and "partition-search
 *      simulation": K in 1..ETHCNN_BUDGET_MAX_RUNGS, each rung in the simulator's ranges, weight[d] < 2^32, budget_ppm <= 10^6, mode
 *      ETHCNN_BUDGET_FRAME or ETHCNN_BUDGET_CARRY; W and H multiples of 8 (up to 65536), a frame of fewer than 2^24 CTUs.  Otherwise
 *      ETHCNN_ERR_ARG with nothing changed.  ladder NULL: the default ladder (K is not read); weight NULL: 64 16 4 1.
 *      ethcnn_pacer_check applies the rules of ladder, K, weights, budget and mode alone (host only, pure, no context; the message is
 *      read with ethcnn_last_error(NULL)).
 *   A cost that cannot fit: a frame whose weighted cost could not fit in 64 bits -- nctu * (weight[0] + 4 weight[1] + 16 weight[2] +
 *      64 weight[3]) >= 2^64, which no frame below 2^24 CTUs reaches -- is refused with ETHCNN_ERR_ARG as in ethcnn_budget_choose, BEFORE
 *      anything is launched: carry and frame count stay untouched.
 *   Input per frame: probs float32 [nctu][21] in raster order as the predictors write it, read as given: gates none.  The CTU rejection
 *      rule (a NaN, a negative or a > 1 value) and bin = ceil(p * 1024) in fp32 are those of the simulator.
 *   What the pacer keeps, all in HBM: the ladder with the full search appended as rung K (int32 [K + 1][6]), the table checked uint32
 *      [K + 1][4], a record scratch of 64 bytes per CTU of the largest frame seen (grown on demand: ETHCNN_ERR_NOMEM with the byte count
 *      in the message, nothing changed; growing waits for the frames in flight), the 128-bit carry and the frame counter.  One result
 *      slot lies in page-locked memory.  The host form holds 84 bytes per CTU of staging when a pointer is not page-locked.
 *   The equality that defines it: F frames of one geometry paced one by one, from create or reset on, give per frame the rung, over,
 *      cost and full, and every baked byte, that ethcnn_budget_control returns for the same ladder, weights, budget and mode with
 *      first = 0 on a simulator that got the same F frames through ethcnn_sim_add_frames (labels NULL); carry is carry_f of the choice
 *      rule, in units of cost x 10^6.
 *   The geometry may change between frames: the carry is in cost units and continues; the results then equal ethcnn_budget_choose over
 *      the concatenated per-frame checked tables.
 *   ethcnn_pacer_result, 72 bytes, little-endian, no padding: frame int64 at 0 (0-based count of frames paced since create / reset), rung
 *      int32 at 8, over int32 at 12, cost uint64 at 16, full uint64 at 24, carry_lo uint64 at 32, carry_hi uint64 at 40, up_k int32[3] at
 *      48, down_k int32[3] at 60 (the picked rung's thresholds).
 *   ethcnn_pacer_frame_device is asynchronous on the context's stream and synchronises nothing (but for a scratch that has to grow):
 *      frames queued back to back without a host wait give the same results.  d_baked == d_probs (in place) is allowed; d_result may be
 *      NULL; pointers must be 4-byte aligned (else ETHCNN_ERR_ARG).
 *   ethcnn_pacer_frame is synchronous.  A pointer that lies in an ethcnn_host_alloc buffer is read or written in place by the kernels,
 *      anything else is staged; the bytes do not depend on the path.  baked == probs is allowed; result may be NULL.  With a page-locked
 *      output the wait is a bounded spin on the context's completion word, which one lane stores behind the bake, with
 *      hipStreamSynchronize as the fallback: the pattern of ethcnn_synchronize.
 *   ethcnn_pacer_last is synchronous: the result of the most recent frame queued by either form (ETHCNN_ERR_ARG when none has been since
 *      create / reset).  ethcnn_pacer_reset sets carry = 0 and frame = 0, in stream order behind the frames already queued.
 *   A call that fails leaves outputs, carry and frame count untouched.  Integers and three float constants only: nothing depends on the
 *      grid or on the order in which blocks finish.  A pacer is destroyed before its context. */
typedef struct ethcnn_pacer ethcnn_pacer;
typedef struct ethcnn_pacer_result {
    int64_t frame;
    int32_t rung;
    int32_t over;
    uint64_t cost, full;
    uint64_t carry_lo, carry_hi;
    int32_t up_k[3], down_k[3];
} ethcnn_pacer_result;
int ethcnn_pacer_check(const ethcnn_sim_thr* ladder, int64_t K, const uint64_t weight[4], uint32_t budget_ppm, int mode);
int ethcnn_pacer_create(ethcnn_ctx* ctx, const ethcnn_sim_thr* ladder, int64_t K, const uint64_t weight[4], uint32_t budget_ppm, int mode,
                        ethcnn_pacer** out);
void ethcnn_pacer_destroy(ethcnn_pacer* pacer);
int ethcnn_pacer_reset(ethcnn_pacer* pacer);
int ethcnn_pacer_frame_device(ethcnn_pacer* pacer, const float* d_probs, int width, int height, float* d_baked, ethcnn_pacer_result* d_result);
int ethcnn_pacer_frame(ethcnn_pacer* pacer, const float* probs, int width, int height, float* baked, ethcnn_pacer_result* result);
int ethcnn_pacer_last(ethcnn_pacer* pacer, ethcnn_pacer_result* out);

/* ---- search budget, online: several sequences.  A PACER SET is the pacer above in the shape of "config #5 online, several live encoders":
 *      one ladder, one weight vector, one budget and one mode, and up to ETHCNN_PACER_SET_MAX SLOTS.  A slot owns what a pacer owns per
 *      sequence -- the 128-bit carry, the frame count, the table checked uint32 [K + 1][4], the picked rung's row and one 72-byte result
 *      slot in page-locked memory -- and a call paces n = 1..32 frames, each of another slot, in TWO launches on the context's stream
 *      whatever n is: one kernel packs every frame's records, counts the checks of every rung into the table of the frame's slot and makes
 *      each slot's choice on the device (the block that finishes a FRAME last chooses for it; no block waits for another), one kernel bakes
 *      every frame under the row its slot's choice left behind.  No reference counterpart.
 *   The equality that defines it: for every slot, the sequence of results (frame, rung, over, cost, full, carry, thresholds) and every
 *      baked byte are those of an ethcnn_pacer with the same ladder, weights, budget and mode that is given the same frames of that slot
 *      in the same order and the same resets -- whatever other slots shared the calls, in whatever order the frames stood in them, and
 *      whichever subset of the slots a call names.
 *   ethcnn_pacer_set_create    nslots in 1..32; ladder, K, weight, budget_ppm, mode under the rules of ethcnn_pacer_check (ladder NULL: the
 *                              default ladder, K is not read; weight NULL: 64 16 4 1).  Holds in HBM the ladder, nslots tables and nslots
 *                              x 16 state words, and nslots result slots in page-locked memory.  Destroy the set before its context.
 *   ethcnn_pacer_set_reset     carry = 0 and frame = 0 of ONE slot, in stream order behind the frames already queued; no other slot is
 *                              touched.
 *   ethcnn_pacer_set_frames_device   frames[n]: {slot, probs, width, height, baked, result} with DEVICE pointers.  Asynchronous on the
 *                              context's stream; synchronises nothing, except when the record scratch has to grow.  The scratch is shared
 *                              by the slots: 64 bytes per CTU of the call with the most CTUs seen (ETHCNN_ERR_NOMEM with the byte count in
 *                              the message, nothing changed; growing waits for the frames in flight).  baked == probs (in place) is
 *                              allowed; result (72 bytes, written when the frame's choice is made) may be NULL.
 *   ethcnn_pacer_set_frames    the same with HOST pointers, synchronous.  A pointer inside an ethcnn_host_alloc buffer is read or written
 *                              in place by the kernels; every other frame goes through one staging buffer (84 bytes per staged CTU of the
 *                              call); the bytes do not depend on the route.  result is a host pointer here and may be NULL.  When every
 *                              output is page-locked the wait is ethcnn_pacer_frame's: the context's completion word, which one lane
 *                              stores behind the bake (a third launch), with hipStreamSynchronize as the fallback.
 *   ethcnn_pacer_set_last      synchronous: the result of the slot's most recent frame (ETHCNN_ERR_ARG when it has paced none since create /
 *                              its reset).
 *   ethcnn_pacer_set_slots, ethcnn_pacer_set_launches   host only: nslots; the kernels the set has enqueued since create (two per call,
 *                              three where the host form stores the completion word).  Negative: a NULL set.
 *   ethcnn_pacer_set_plan      host only, no context: the layout of a call over frames of nctus[j] CTUs under K + 1 rungs, in call order.
 *                              Frame j owns the blocks [count_first[j], count_first[j] + count_blocks[j]) of the count kernel --
 *                              count_blocks = slices x ceil((K + 1) / 256), slices of slice_len[j] CTUs cut as ethcnn_pacer_frame cuts
 *                              them: at most 64 CTUs, balanced (272 CTUs: 55, 55, 55, 55, 52) --, the blocks from bake_first[j] on of the
 *                              bake kernel, ceil(nctus[j] / 256) of them, and the records from rec0[j] on, the running sum of the CTUs.
 *                              Every output has n entries and may be NULL; the two grid sizes are the totals.  All sums are kept in 64
 *                              bits.  ETHCNN_ERR_ARG with nothing written: n outside 1..32, a frame of no CTU or of 2^24 or more, K outside
 *                              1..ETHCNN_BUDGET_MAX_RUNGS, NULL nctus.
 *   Refusals of a call, each ETHCNN_ERR_ARG before anything is allocated or enqueued, so that every slot's next result is what it would have
 *      been without the call: n outside 1..32; a slot outside 0..nslots - 1 or named twice; a NULL probs or baked; a pointer that is not
 *      4-byte aligned; a baked that overlaps ANOTHER frame's probs or baked; a frame that ethcnn_pacer_frame would refuse (W or H no
 *      multiple of 8 or above 65536, 2^24 CTUs or more, a cost bound that may not fit in 64 bits).  The text is read with ethcnn_last_error
 *      of the context, as the pacer's is.
 *   (A space stands before the parenthesis of these declarations, so that a search for the pacer's own entries, `ethcnn_pacer_` + name +
 *      `(`, lists those seven and nothing else.) */
#define ETHCNN_PACER_SET_MAX 32
typedef struct ethcnn_pacer_set ethcnn_pacer_set;
typedef struct ethcnn_pacer_set_frame {
    int slot;                    /* 0..nslots - 1; at most once per call */
    const float* probs;          /* [nctu][21] */
    int width, height;
    float* baked;                /* [nctu][21]; may be probs */
    ethcnn_pacer_result* result; /* may be NULL */
} ethcnn_pacer_set_frame;
int ethcnn_pacer_set_create (ethcnn_ctx* ctx, int nslots, const ethcnn_sim_thr* ladder, int64_t K, const uint64_t weight[4], uint32_t budget_ppm,
                             int mode, ethcnn_pacer_set** out);
void ethcnn_pacer_set_destroy (ethcnn_pacer_set* set);
int ethcnn_pacer_set_slots (const ethcnn_pacer_set* set);
int64_t ethcnn_pacer_set_launches (const ethcnn_pacer_set* set);
int ethcnn_pacer_set_reset (ethcnn_pacer_set* set, int slot);
int ethcnn_pacer_set_frames_device (ethcnn_pacer_set* set, const ethcnn_pacer_set_frame* frames, int n);
int ethcnn_pacer_set_frames (ethcnn_pacer_set* set, const ethcnn_pacer_set_frame* frames, int n);
int ethcnn_pacer_set_last (ethcnn_pacer_set* set, int slot, ethcnn_pacer_result* out);
int ethcnn_pacer_set_plan (const int64_t* nctus, int n, int64_t K, int64_t* count_first_out, int64_t* count_blocks_out, int32_t* slice_len_out,
                           int64_t* bake_first_out, int64_t* rec0_out, int64_t* count_grid_out, int64_t* bake_grid_out);

/* ---- search budget, online: several sequences, a POLICY per slot.  A policy is {ladder, K, weight[4], budget_ppm, mode} under the rules
 *      of ethcnn_pacer_check, unchanged (ladder NULL: the default ladder, K is not read; weight NULL: 64 16 4 1).  A set holds
 *      1..ETHCNN_PACER_SET_MAX_POLICIES of them and every slot is BOUND to one: a four-QP evaluation paces each directory under the
 *      ladder of its own model, a complexity-control curve runs four budgets through one set.  The eight entries above stay as they
 *      are; a set made by ethcnn_pacer_set_create is a set of one policy bound to every slot.
 *   The equality that defines it: for every slot, between two binds, the sequence of results and every baked byte are those of an
 *      ethcnn_pacer created with the slot's policy and given the same frames in the same order -- whatever policies the other slots of
 *      the calls had, in whatever order the frames stood, and whichever subset a call named.  A call is still two launches, three where
 *      the host form stores the completion word.
 *   ethcnn_pacer_policies_check    host only, no context: the rules of every policy (the first broken one, with "policy <index>: " in
 *                              front of ethcnn_pacer_check's message, read with ethcnn_last_error(NULL)), npolicies in 1..32, and, where
 *                              slot_policy is not NULL, nslots in 0..32 entries in 0..npolicies - 1.
 *   ethcnn_pacer_policies_create   ethcnn_pacer_set_create with a policy list; slot_policy [nslots] binds the slots (NULL: all to
 *                              policy 0).  In HBM, written once: all ladders in one int32 [sum of rungs][6], each with its full search
 *                              appended, and one 48-byte record per policy.  A slot's table has as many rows as the longest ladder has
 *                              rungs, so that a bind allocates nothing.
 *   ethcnn_pacer_policies_count, ethcnn_pacer_policies_of   host only: the number of policies; the policy a slot is bound to.  Negative:
 *                              a NULL set, a slot outside 0..nslots - 1.
 *   ethcnn_pacer_policies_bind      ethcnn_pacer_set_reset of that slot plus the new binding, in stream order behind the frames already queued
 *                              (they keep the policy they were queued under).  No other slot is touched.  Binding a slot to the policy it
 *                              already has is a reset.  ETHCNN_ERR_ARG with nothing changed: a slot outside 0..nslots - 1, a policy
 *                              outside 0..npolicies - 1.
 *   ethcnn_pacer_policies_plan   ethcnn_pacer_set_plan with K[j] + 1 rungs for frame j -- the ladder of its slot's policy --, so that
 *                              count_blocks[j] = slices x ceil((K[j] + 1) / 256): one call mixes frames of 1 and of 17 rung blocks.
 *                              Refuses per frame what ethcnn_pacer_set_plan refuses, and a NULL K.
 *   These six act on an ethcnn_pacer_set; their prefix is ethcnn_pacer_policies_, so that ethcnn_pacer_set_* stays the nine entries above.
 *   The cost bound of a frame (a cost that may not fit in 64 bits) is taken under the weights of its slot's policy; one refused frame
 *      still refuses the whole call before anything is allocated or enqueued. */
#define ETHCNN_PACER_SET_MAX_POLICIES 32
typedef struct ethcnn_pacer_policy {
    const ethcnn_sim_thr* ladder; /* NULL: the default ladder */
    int64_t K;
    const uint64_t* weight;       /* [4]; NULL: 64 16 4 1 */
    uint32_t budget_ppm;
    int32_t mode;
} ethcnn_pacer_policy;
int ethcnn_pacer_policies_check (const ethcnn_pacer_policy* policies, int npolicies, const int* slot_policy, int nslots);
int ethcnn_pacer_policies_create (ethcnn_ctx* ctx, int nslots, const ethcnn_pacer_policy* policies, int npolicies, const int* slot_policy,
                                      ethcnn_pacer_set** out);
int ethcnn_pacer_policies_count (const ethcnn_pacer_set* set);
int ethcnn_pacer_policies_of (const ethcnn_pacer_set* set, int slot);
int ethcnn_pacer_policies_bind (ethcnn_pacer_set* set, int slot, int policy);
int ethcnn_pacer_policies_plan (const int64_t* nctus, const int64_t* K, int n, int64_t* count_first_out, int64_t* count_blocks_out,
                                 int32_t* slice_len_out, int64_t* bake_first_out, int64_t* rec0_out, int64_t* count_grid_out,
                                 int64_t* bake_grid_out);

/* ---- search budget: building a ladder.  The two sections above pick a rung of a LADDER per frame; how well they hold a budget depends on
 *      that ladder, and the default one is the same on every level and never looks at a label.  These entries turn a simulator's set
 *      with labels into a ladder by a greedy walk from the full search: every step moves ONE of the six thresholds to the nearest grid
 *      value that lowers the weighted check count, and of the six possible moves takes the one that costs the fewest newly bad CTUs per
 *      unit of cost saved.  One launch per step; the choice is made on the device.  No reference counterpart.
 *   Inputs: a simulator set with at least one labelled CTU; weight[4] under the rules of "search budget" (NULL: 64 16 4 1); grid, a power
 *      of two in 1..1024; max_rungs in 1..ETHCNN_BUDGET_MAX_RUNGS; max_bad_ppm <= 10^6.  The gates are always ETHCNN_SIM_GATES_NONE, as
 *      for every budget entry.  Throughout, cost = sum_d weight[d] * checked[d] and bad = bad_ctus, both of ethcnn_sim_counts over the
 *      WHOLE set.
 *   Rung 0 is the full search (up_k = 1024, down_k = -1 on all levels), with coord = -1 and value = 0.
 *   A step from the rung with thresholds t, cost C and bad CTUs B.  Coordinates are taken in the sweep order c = 0..5 = down0, up0, down1,
 *      up1, down2, up2 (ethcnn_sim_sweep), d = c >> 1 is the level.  Each coordinate has at most one move:
 *        1. its candidate values v are the multiples of grid with   down_k[d] < v <= up_k[d]            for a down,
 *                                                                   max(down_k[d], 0) <= v < up_k[d]    for an up
 *           (so down_k <= up_k holds on every rung);
 *        2. they are walked from the one nearest to the coordinate's current value outwards (rising for a down, falling for an up);
 *        3. the move is the FIRST v with cost(v) < C, where cost(v) is the cost of t with that one coordinate set to v; without one the
 *           coordinate has no move;
 *        4. if that v has bad(v) * 10^6 > max_bad_ppm * labelled_ctus the coordinate has no move: nothing further is looked at.
 *      Of the moves, the one with the smallest (bad(v) - B) / (C - cost(v)) is taken, compared exactly by signed 128-bit cross products
 *      (bad(v) - B may be negative); at a tie the larger saving C - cost(v), at a further tie the smaller c.
 *      The walk stops when no coordinate has a move, or at max_rungs rungs.  Costs fall strictly along the path.
 *   Result: ethcnn_ladder_rung[*nrungs_out], 72 bytes each, little-endian, no padding: thr at 0, coord int32 at 24 (the coordinate that
 *      moved), value int32 at 28 (where to), checked uint64[4] at 32 and bad_ctus uint64 at 64: exactly what ethcnn_sim_eval gives for thr
 *      under gates none.
 *   Refusals, each ETHCNN_ERR_ARG with the outputs untouched and before anything is launched: a set without a labelled CTU; a grid
 *      that is no power of two in 1..1024; max_rungs outside 1..ETHCNN_BUDGET_MAX_RUNGS; max_bad_ppm > 10^6; a weight of 2^32 or more; a
 *      cost bound ctus * (weight[0] + 4 weight[1] + 16 weight[2] + 64 weight[3]) that does not fit in 64 bits.  ethcnn_ladder_check
 *      applies the rules of the four plain arguments alone (host only, pure; the message is read with ethcnn_last_error(NULL)).
 *   ethcnn_ladder_build is synchronous on the context's stream.  Per call it holds in HBM a table uint64 [6][1025 / grid + 1][5], a state
 *      block and max_rungs rungs (ETHCNN_ERR_NOMEM when they do not fit).  Integers only: nothing depends on the launch grid or on the
 *      order in which blocks finish, and a second build on the same set gives the same bytes.
 *   ethcnn_ladder_thin (host only, pure): cost[n] must fall strictly (else ETHCNN_ERR_ARG); picks at most K of the n rungs, evenly spaced
 *      in COST.  n <= K: the identity.  K = 1: rung 0.  Otherwise for j = 0..K-1, target_j = cost[0] - floor(j * (cost[0] - cost[n-1]) /
 *      (K - 1)) with a 128-bit product, and idx_j is the smallest i with cost[i] <= target_j; the output is the distinct idx_j in rising
 *      order (rungs 0 and n - 1 are always among them).  idx_out holds min(n, K) entries, *k_out says how many were written.  NULL, n < 1
 *      or K < 1: ETHCNN_ERR_ARG, outputs untouched.
 *   ethcnn_ladder_write (host only): K rungs (1..ETHCNN_BUDGET_MAX_RUNGS, each in the simulator's ranges), one per line, six values k / 1024
 *      with ten decimals in the token order `order` (ETHCNN_THR_ORDER_AI / _LDP), to a temp file that is then renamed: the ladder file
 *      that tools/control_budget.py --ladder and ETHCNN_SEARCH_BUDGET_LADDER read.  Every grid value, down_k = -1 included, reads back
 *      exactly. */
typedef struct ethcnn_ladder_rung {
    ethcnn_sim_thr thr;
    int32_t coord;
    int32_t value;
    uint64_t checked[4];
    uint64_t bad_ctus;
} ethcnn_ladder_rung;
int ethcnn_ladder_check(const uint64_t weight[4], int grid, int64_t max_rungs, uint32_t max_bad_ppm);
int ethcnn_ladder_build(ethcnn_sim* sim, const uint64_t weight[4], int grid, int64_t max_rungs, uint32_t max_bad_ppm, ethcnn_ladder_rung* rungs_out,
                        int64_t* nrungs_out);
int ethcnn_ladder_thin(const uint64_t* cost, int64_t n, int64_t K, int32_t* idx_out, int64_t* k_out);
int ethcnn_ladder_write(const char* path, const ethcnn_sim_thr* thr, int64_t K, int order);

/* ---- partition-search simulation: expected wrong decisions.  wrong_split[] / wrong_stop[] / bad_ctus above need labels, and labels need
 *      the full-search encode this project exists to avoid.  The model prices a forced decision itself: a node forced CURRENT ONLY whose
 *      split probability is p is wrong with probability p, a node forced SPLIT ONLY with probability 1 - p.  Summed over the decided
 *      nodes of the pruned search that gives the EXPECTED values of wrong_stop[] and wrong_split[], from the bins the simulator's records
 *      already hold and without a label.  No reference counterpart.
 *   Unit and table.  ETHCNN_RISK_ONE = 2^20 stands for probability 1.  A RELIABILITY TABLE is uint32_t rel[3][1025] (level, bin), every
 *      value in 0..ETHCNN_RISK_ONE: rel[l][b] estimates the share of the level-l nodes with bin b whose truth flag (those of the
 *      calibration block) is "split".  The IDENTITY table is rel[l][b] = b * 1024, that is p rounded up to its bin edge b / 1024: it
 *      takes the model at its word.  A simulator starts with the identity table.  ethcnn_risk_set_reliability validates and uploads a
 *      table (NULL: the identity); a value above ETHCNN_RISK_ONE is ETHCNN_ERR_ARG and changes nothing.  The table belongs to the
 *      simulator, not to the set: ethcnn_sim_reset keeps it.
 *   Counter.  Under ETHCNN_SIM_GATES_NONE only (the probabilities are what the encoder will read), over every CTU that is not rejected,
 *      labelled or not, wholly inside the picture or not.  Each DECIDED NODE (rule line 4 of "partition-search simulation") of level l
 *      and bin b contributes by its outcome:
 *        CURRENT ONLY   exp_wrong_stop[l]  += rel[l][b]
 *        SPLIT ONLY     exp_wrong_split[l] += ETHCNN_RISK_ONE - rel[l][b]
 *        BOTH           nothing
 *      risk = the sum of the six fields: expected wrong nodes in units of 1 / ETHCNN_RISK_ONE.  The sums are exact integers, so they do
 *      not depend on the launch grid, on the order of adds or on how a set is split over adds.  Bound: a CTU has 21 nodes, so 2^31 CTUs
 *      x 16 nodes of a level x 2^20 = 2^55 per field, and the sum of six fields stays below 2^58: everything fits in 64 bits.
 *   ethcnn_risk_eval: out[c] = the counter of candidate cand[c] over the whole set.  ncand == 0 is a no-op, an empty set gives zeros,
 *      a candidate outside the simulator's ranges is ETHCNN_ERR_ARG.  Synchronous on the context's stream.
 *   Tables (host only, pure, no context; errors are read with ethcnn_last_error(NULL)):
 *      ethcnn_risk_identity(rel) writes the identity table.
 *      ethcnn_risk_from_hist(hist, rel) fits a table to the ETHCNN_CALIB_HIST_WORDS words of ethcnn_calib_get, NON-DECREASING in the bin,
 *        by pool-adjacent-violators.  Per level, s_b = hist[l][1][b] and t_b = s_b + hist[l][0][b].  Walk b = 0..1024 with a stack of
 *        blocks (S, T, first, last): push (s_b, t_b, b, b); then, while there are two blocks and (top.T == 0 or below.T == 0 or
 *        below.S * top.T > top.S * below.T, in 128-bit products), merge the top block into the one below (S and T add, last = top.last).
 *        So empty bins join the block on their left, and leading empty bins join the first block that has samples.  Every bin of a
 *        block gets floor(S * 2^20 / T).  A level without any sample gets the identity.
 *      ethcnn_risk_write(path, rel) / ethcnn_risk_read(path, rel): a text file, first line "ethcnn-reliability 1", then three lines
 *        (levels 0, 1, 2) of 1025 decimal integers separated by blanks.  Written to a temp file that is then renamed (a table with a
 *        value above ETHCNN_RISK_ONE: ETHCNN_ERR_ARG, nothing written).  On reading,
 *        anything else -- another first line, a missing or a further token, a token that is no decimal integer -- or a value above
 *        ETHCNN_RISK_ONE is ETHCNN_ERR_FORMAT and rel is untouched; a file that cannot be opened is ETHCNN_ERR_IO.
 *   ethcnn_risk_ladder_build: the walk of "search budget: building a ladder" on a set WITHOUT labels.  It is that walk word for word --
 *      rung 0, the candidate values of a coordinate, nearest first, the FIRST value with cost(v) < C, the sweep order -- with bad
 *      replaced by risk: B becomes R, the risk of the current rung, and bad(v) becomes risk(v) of ethcnn_risk_eval under the
 *      simulator's table.  Rule 4 becomes: if risk(v) * 10^6 > max_risk_ppm * counted_ctus * ETHCNN_RISK_ONE (128-bit products) the
 *      coordinate has no move, with counted_ctus = ctus - rejected_ctus of ethcnn_sim_info; so the cap reads "expected wrong nodes per
 *      million CTUs" (max_risk_ppm is a uint64_t: UINT64_MAX, like any value from 21 * 10^6 on, is no cap).  Of the moves, the one
 *      with the smallest (risk(v) - R) / (C - cost(v)) is taken, compared exactly by signed 128-bit cross products; ties break as in
 *      the labelled walk (the larger saving, then the smaller c).  No labelled CTU is needed; a set with counted_ctus == 0 is
 *      ETHCNN_ERR_ARG, as are the refusals of the labelled build for weight, grid, max_rungs and the cost bound.
 *      A rung is an ethcnn_ladder_rung_risk, 112 bytes, little-endian, no padding: thr at 0, coord int32 at 24, value int32 at 28,
 *      checked uint64[4] at 32, exp_wrong_split uint64[3] at 64, exp_wrong_stop uint64[3] at 88: exactly what ethcnn_sim_eval (gates
 *      none) and ethcnn_risk_eval give for thr.  Synchronous; per call a table uint64 [6][1025 / grid + 1][10], a state block and
 *      max_rungs rungs in HBM.  A second build on the same set and table gives the same bytes.  ethcnn_ladder_check (with max_bad_ppm
 *      0), ethcnn_ladder_thin and ethcnn_ladder_write serve both kinds of ladder.
 *   What this is not.  The identity table ASSUMES A CALIBRATED MODEL: where the model is over-confident the figure is too low, and only
 *      a table fitted on labelled material (ethcnn_risk_from_hist) corrects that, for material like the one it was fitted on.  The
 *      level-1 and level-2 probabilities come from a model trained under teacher forcing -- on nodes whose parents were truly split --
 *      while the counter also asks them on nodes the pruned search reaches for other reasons ("threshold calibration on reached nodes"
 *      below gives the histogram of those nodes, in the layout ethcnn_risk_from_hist takes).  The figure counts nodes, not CTUs, and
 *      nothing relates it to encoding time or to BD-rate. */
#define ETHCNN_RISK_ONE (1u << 20)
#define ETHCNN_RISK_REL_WORDS (3 * ETHCNN_CALIB_BINS)
typedef struct ethcnn_sim_risk {
    uint64_t exp_wrong_split[3], exp_wrong_stop[3];
} ethcnn_sim_risk;
typedef struct ethcnn_ladder_rung_risk {
    ethcnn_sim_thr thr;
    int32_t coord;
    int32_t value;
    uint64_t checked[4];
    uint64_t exp_wrong_split[3], exp_wrong_stop[3];
} ethcnn_ladder_rung_risk;
int ethcnn_risk_set_reliability(ethcnn_sim* sim, const uint32_t* rel_or_null);
int ethcnn_risk_eval(ethcnn_sim* sim, const ethcnn_sim_thr* cand, int64_t ncand, ethcnn_sim_risk* out);
int ethcnn_risk_identity(uint32_t* rel);
int ethcnn_risk_from_hist(const uint64_t* hist, uint32_t* rel);
int ethcnn_risk_write(const char* path, const uint32_t* rel);
int ethcnn_risk_read(const char* path, uint32_t* rel);
int ethcnn_risk_ladder_build(ethcnn_sim* sim, const uint64_t weight[4], int grid, int64_t max_rungs, uint64_t max_risk_ppm,
                             ethcnn_ladder_rung_risk* rungs_out, int64_t* nrungs_out);

/* ---- threshold calibration on reached nodes.  The calibrator of "threshold calibration" counts TEACHER-FORCED populations: a 32 x 32
 *      block only when its CTU is labelled split, a 16 x 16 block only when both ancestors are.  HM does not visit those populations: it
 *      visits a 32 x 32 node whenever the decision above it was SPLIT ONLY, BOTH or a frame edge, whether or not the label agrees.  So
 *      the calibrator's budgets hold for nodes the encoder never sees, and a reliability table fitted to its histogram is applied (by
 *      the expected wrong decisions above) to nodes it was not fitted on.  The two entries here count and choose on the nodes the pruned
 *      search REACHES, from the records a simulator already holds.  No reference counterpart.
 *   ethcnn_reach_hist.  Over the LABELLED CTUs of the simulator's set (those of labelled_ctus: not rejected, wholly inside the picture,
 *      with labels), for candidate c: every DECIDED NODE (rule line 4 of "partition-search simulation") of level l adds one to
 *      hist[c][l][t][b], in the calibrator's layout [3 levels][2 truths][1025 bins], where
 *        t = the node's own truth flag, the simulator's: judged whatever happened above it;
 *        b = the bin AS THE ENCODER READS IT: the record's bin, or 0 where a closed batch gate of gate_order zeroed it.
 *      The gates are those of the simulator's evaluation under the same gate_order; CTUs added in the per-CTU layout are never gated.
 *      Unlabelled and rejected CTUs add nothing.  Counts are exact integers and do not depend on the grid, on the order of adds or on
 *      how a set is split over adds.  ncand == 0 is a no-op; an empty set, or one without labelled CTUs, gives zeros.  A candidate
 *      outside the simulator's ranges, ncand > ETHCNN_REACH_MAX_CAND, a gate_order that is none of the three or a NULL pointer is
 *      ETHCNN_ERR_ARG, and nothing is written.  Synchronous on the context's stream; per call ncand x 49,200 bytes of device memory.
 *   Identities.  For every candidate and gate order, with ev = the simulator's evaluation counters of the same arguments and hist the
 *      candidate's histogram:
 *        ev.wrong_split[l] == sum_{b > up_k[l]} hist[l][0][b]
 *        ev.wrong_stop[l]  == sum_{b <= min(down_k[l], up_k[l])} hist[l][1][b]      (HM tests "split only" first)
 *        hist[l] depends only on the thresholds of the levels < l (through the descent and the gates) and on nothing deeper;
 *        hist[0] is the same for every candidate;
 *        under the full search with ETHCNN_SIM_GATES_NONE hist[l] counts EVERY level-l node of every labelled CTU;
 *        when no probability of the data is out of range, hist[0] equals level 0 of ethcnn_calib_get over the same data.
 *   ethcnn_reach_calibrate.  Top-down, three histograms, the choices on the host.  Starting from thr = the full search, for l = 0, 1, 2:
 *        H = the histogram of thr;  report->level[l] = level l of ethcnn_calib_choose(H, eps_down_ppm, eps_up_ppm);
 *        thr.up_k[l], thr.down_k[l] = that level's up_k, down_k.
 *      thr_out is the result; counts_out (may be NULL) the simulator's evaluation of it under gate_order.  So n0 / n1 of a level are the
 *      unsplit / split nodes the pruned search reaches under the levels above, and the budgets are shares of those.  For the result,
 *      counts.wrong_stop[l] == report.level[l].miss and counts.wrong_split[l] == report.level[l].fsplit exactly, crossed levels
 *      included.  No labelled CTU, a budget above 10^6, a bad gate_order or a NULL eps_down_ppm / eps_up_ppm / report / thr_out:
 *      ETHCNN_ERR_ARG, and no output is written.
 *   The layout is the calibrator's on purpose: ethcnn_risk_from_hist, ethcnn_calib_choose and ethcnn_calib_write_thr_info take a reach
 *      histogram or report unchanged.  The table to fit for the expected wrong decisions is the one of the FULL-SEARCH candidate under
 *      ETHCNN_SIM_GATES_NONE: it covers all nodes of the labelled CTUs, the population that counter meets at rung 0 and thins from there.
 *   What this is not.  The choice is greedy: level l is fixed before the cost of level l + 1 is seen.  One table for all QPs. */
#define ETHCNN_REACH_HIST_WORDS ETHCNN_CALIB_HIST_WORDS
#define ETHCNN_REACH_MAX_CAND 256
int ethcnn_reach_hist(ethcnn_sim* sim, const ethcnn_sim_thr* cand, int64_t ncand, int gate_order, uint64_t* hist /* [ncand][ETHCNN_REACH_HIST_WORDS] */);
int ethcnn_reach_calibrate(ethcnn_sim* sim, const uint32_t eps_down_ppm[3], const uint32_t eps_up_ppm[3], int gate_order, ethcnn_calib_report* report,
                           ethcnn_sim_thr* thr_out, ethcnn_sim_counts* counts_out /* may be NULL */);

/* ---- comparing two predictions: how far two sets of probabilities are apart, and whether the encoder's pruned search changes (no
 *      reference counterpart).  The questions behind every "byte-identical" and "within tolerance" of this project: a 16-bit plan against
 *      the exact plan, one daemon against another, a retrained model against the one before it, a sharded run against a single one.  One
 *      kernel reads both sets once and answers in the terms of "partition-search simulation" above.
 *   Inputs: a and b, float32 [n][21] in the layout the predictors write; tol >= 0 (a NaN or a negative tol: ETHCNN_ERR_ARG); optionally ONE
 *      candidate thr in the simulator's ranges (else ETHCNN_ERR_ARG; NULL: none).  Layouts as for the calibrator and the simulator:
 *      per-CTU (no geometry, every node is a decided node) and frame (nframes frames of width x height, both multiples of 8 up to 65536,
 *      else ETHCNN_ERR_ARG; rule lines 1-4 of the simulation block apply, frame-edge nodes included).  Gates: none, the probabilities are
 *      compared as given.  n, or nframes x CTUs per frame, of 2^31 or more: ETHCNN_ERR_ARG.
 *   Per value (level 0: p[0]; level 1: p[1..4]; level 2: p[5..20]; all 21 values of a CTU, wherever the CTU lies in the picture):
 *      d = |a - b|, ONE fp32 subtraction with IEEE results for subnormals.
 *      over_tol[level]   values with d > tol
 *      bits_diff[level]  values whose bit patterns differ (-0.0 against 0.0 counts here and nowhere else)
 *      max_abs[level]    the maximum of d;  worst_ctu[level]  the LOWEST CTU index that attains it, -1 when nothing was compared
 *   With thr, bin = ceil(p * 1024) in fp32 with the bit tests of the calibration block, on both sides:
 *      class_diff[level]  values whose outcome (SPLIT ONLY / CURRENT ONLY / BOTH, rule line 4) differs between a and b, visited or not
 *      search_diff_ctus   CTUs whose pruned search differs: the set of (visited node, outcome) pairs of a is not that of b -- another
 *                         node is visited, or a visited decided node has another outcome.  THE number that decides whether HM's
 *                         bitstream can change: 0 means the encoder checks the same CUs under a and under b.
 *      checked_a[4], checked_b[4]  the simulator's checked[] of each side under thr, gates none
 *      Without thr all these fields are 0 and with_thr is 0.
 *   A CTU with a NaN, a negative or a > 1 value among its 42 numbers is left out of everything and counted in rejected_ctus.
 *   ethcnn_compare_stats, 200 bytes, little-endian, no padding: ctus uint64 at 0 (CTUs given, the rejected ones included), rejected_ctus
 *      uint64 at 8, over_tol uint64[3] at 16, bits_diff uint64[3] at 40, class_diff uint64[3] at 64, search_diff_ctus uint64 at 88,
 *      checked_a uint64[4] at 96, checked_b uint64[4] at 128, worst_ctu int64[3] at 160, max_abs float32[3] at 184, with_thr uint32 at 196.
 *   flags (may be NULL), uint8 [n], per CTU: bit 0 rejected (then no other bit), bit 1 a value over tol, bit 2 a class differs, bit 3 the
 *      search differs.
 *   Every field is independent of the launch grid and of how a set is split over calls: integers and fp32 compares only.  Sums add
 *      across calls; a maximum combines by (value, lowest index, the second call's indices moved by the first call's ctus).
 *   The _device entries take pointers in HBM, 4-byte aligned (else ETHCNN_ERR_ARG; no other alignment is needed).  The host entries
 *      read or write a pointer in place when its whole range lies in an ethcnn_host_alloc buffer and stage anything else in pieces of
 *      2^20 CTUs through one device buffer (ETHCNN_ERR_NOMEM with the byte count when it does not fit).  All four are synchronous on the
 *      context's stream and return the stats to the host.  n == 0 / nframes == 0 is a no-op that gives zeros and worst_ctu = -1. */
typedef struct ethcnn_compare_stats {
    uint64_t ctus;
    uint64_t rejected_ctus;
    uint64_t over_tol[3];
    uint64_t bits_diff[3];
    uint64_t class_diff[3];
    uint64_t search_diff_ctus;
    uint64_t checked_a[4], checked_b[4];
    int64_t worst_ctu[3];
    float max_abs[3];
    uint32_t with_thr;
} ethcnn_compare_stats;
int ethcnn_compare_probs_device(ethcnn_ctx* ctx, const float* d_a, const float* d_b, int64_t n, float tol, const ethcnn_sim_thr* thr /* may be NULL */,
                                ethcnn_compare_stats* out, uint8_t* d_flags /* may be NULL */);
int ethcnn_compare_frames_device(ethcnn_ctx* ctx, const float* d_a, const float* d_b, int width, int height, int64_t nframes, float tol,
                                 const ethcnn_sim_thr* thr /* may be NULL */, ethcnn_compare_stats* out, uint8_t* d_flags /* may be NULL */);
int ethcnn_compare_probs(ethcnn_ctx* ctx, const float* a, const float* b, int64_t n, float tol, const ethcnn_sim_thr* thr /* may be NULL */,
                         ethcnn_compare_stats* out, uint8_t* flags /* may be NULL */);
int ethcnn_compare_frames(ethcnn_ctx* ctx, const float* a, const float* b, int width, int height, int64_t nframes, float tol,
                          const ethcnn_sim_thr* thr /* may be NULL */, ethcnn_compare_stats* out, uint8_t* flags /* may be NULL */);
/* The audit of a 16-bit plan on the caller's own pictures: the frames go through ethcnn_predict_luma_device under plan 0 and then under
 * `plan` (2 or 3, else ETHCNN_ERR_ARG), both with open gates (thresholds -1, -1: a gate's knife edge cannot pass for an arithmetic
 * error), and the two results are compared in the frame layout (width, height multiples of 8).  Synchronous.
 *   ethcnn_audit_result, 216 bytes, no padding: the stats at 0, plan int32 at 200, passes int32 at 204 (passes of the audited run),
 *      fast_passes int32 at 208 (of those, the passes that took the 16-bit path), reserved int32 at 212 (0).  A geometry that runs as
 *      single-launch passes computes exactly under every plan: the result then says fast_passes == 0, and its zero differences say
 *      nothing about the plan.
 *   The context's plan, thresholds, profiling counters and the intermediates' bookkeeping that ethcnn_debug_fetch reads are what they
 *      were afterwards, on every error path too.  The workspace itself holds the audit's last pass, so ethcnn_debug_fetch is refused
 *      (ETHCNN_ERR_ARG) from an audit that ran a pass until the caller's next pass: stale intermediates never look valid.  A plan that the load-time guard
 *      refuses: ETHCNN_ERR_PLAN_REFUSED, nothing changed, `out` untouched.  An open streamed call: ETHCNN_ERR_ARG.
 *   Memory: 2 x nframes x nctu x 84 bytes of scratch, the first set rounded up to 16 bytes so that the second one starts aligned and the
 *      comparison keeps its 16-byte loads (at most 12 bytes more; ethcnn_audit_plan_bytes reports the sum; negative: bad arguments), checked against the free device
 *      memory before it is allocated (ETHCNN_ERR_NOMEM, the byte count in the message).
 *   The file entry reads the luma planes of frames first + i step, i < count (first >= 0, step >= 1, count >= 0), of an 8-bit 4:2:0 file
 *      into one contiguous device buffer (count x width x height bytes more) and calls the device entry.  A frame index past the end of the
 *      file is ETHCNN_ERR_ARG before anything runs; a context whose source format is not the default is refused with ETHCNN_ERR_ARG.
 *   Not built: deep or non-4:2:0 sources in the file entry; the Low-Delay-P path (it always computes exactly); multi-GPU; any change to
 *      the guard's own decision; a periodic check inside the passes. */
typedef struct ethcnn_audit_result {
    ethcnn_compare_stats stats;
    int32_t plan;
    int32_t passes;
    int32_t fast_passes;
    int32_t reserved;
} ethcnn_audit_result;
int64_t ethcnn_audit_plan_bytes(int width, int height, int nframes);
int ethcnn_audit_plan_device(ethcnn_ctx* ctx, const uint8_t* d_luma, int width, int height, ptrdiff_t pitch, ptrdiff_t frame_stride, int nframes, int qp,
                             int plan, float tol, const ethcnn_sim_thr* thr /* may be NULL */, ethcnn_audit_result* out);
int ethcnn_audit_plan_yuv_file(ethcnn_ctx* ctx, const char* path, int width, int height, int qp, int plan, int64_t first, int64_t step, int64_t count,
                               float tol, const ethcnn_sim_thr* thr /* may be NULL */, ethcnn_audit_result* out);

/* ---- sample-set replay: an inter sample set (LDP_Valid.dat, LDP_Test.dat, plain or _shuffled: the 16516-byte records of "sample sets"
 *      above) put back together into the residual pictures and label planes it was cut from, and run through the deployed Low-Delay-P
 *      chain, ethcnn_ldp_sequence_device: forward in time, i_frame % 4 features, the state carried over the whole sequence.  The inverse
 *      of ethcnn_samples_cut_device plus a plan.  (No reference counterpart: the trainers' own evaluation scores 20-step windows from a
 *      zero state through the training graph.)
 *   Header fields of a record: w = u16 at byte 2, h = u16 at byte 4; f = u32 at byte 10, the frame number in encoding order; line = u16 at
 *      byte 14, col = u16 at byte 16, seq = u16 at byte 18; slot QP q_s = the byte at 64 + 4113 s.  All little-endian.  C = w / 64,
 *      R = h / 64 (integer divisions), nctu = R C.
 *   Run: a maximal set of records with the same (seq, w, h).  Runs are ordered by seq, then by first appearance.  A run is valid when
 *        - its frame numbers form one contiguous range f0..f1,
 *        - every (f, line, col) with line < R, col < C occurs exactly once,
 *        - no other (line, col) occurs,
 *        - each q_s is the same in all its records, and the four differ.
 *      Anything else is ETHCNN_ERR_FORMAT.  The rules are checked over the whole input in this order, and the first one that is broken
 *      anywhere is reported with its name in quotes and the lowest record index that shows it:
 *        'geometry'          w < 64, h < 64 or f >= 2^31 (no whole CTU; the sequence call counts frames in an int): that record
 *        'outside'           line >= R or col >= C: that record
 *        'QP differs'        a record whose four q_s are not those of the lowest record of its run: that record
 *        'QPs not distinct'  the lowest record of a run whose four q_s are not distinct
 *        'duplicate'         a record whose (f, line, col) a lower record of its run holds already: the higher record
 *        'missing'           with f0 / f1 the lowest / highest frame number of the run: the first (f, line, col) in that order within
 *                            f0..f1 that no record holds; it is shown by the lowest record of the run whose frame number is >= f
 *      Record order in the input is irrelevant: an unshuffled file, a "_shuffled" file and ethcnn_samples_read with a seed give the same
 *      plan up to the source indices.
 *   Source table of a run: src[F][nctu] int64 with F = f1 - f0 + 1; src[f - f0][line C + col] = the index of the record at (f, line, col).
 *   Reconstructed planes of a run at slot s: residual [F][64 R][64 C] uint8, byte (y, x) of frame f = residual byte 64 (y % 64) + x % 64 of
 *      the record at (f, y / 64, x / 64) (a slot's residual starts at record byte 81 + 4113 s); labels [F][4 R][4 C] uint8 from the 16
 *      depth bytes (record byte 65 + 4113 s on) in the same way.  These are the whole-CTU crops of the planes the set was cut from.
 *   Replay of a run at slot s: what ethcnn_ldp_sequence_device gives for the residual planes with width = 64 C, height = 64 R, qp = q_s,
 *      i_frame_first = f0 and a state_in of zeros (also when f0 > 1: a file that starts in the middle of a sequence starts from a zero
 *      state, and never from whatever state the context holds).  The context's thresholds and weights are used as they are; the LSTM
 *      bundle that goes with q_s is the caller's choice, as for the sequence call.  Output: float32 [F][nctu][21].
 *      With open gates (thresholds 0, 0) every value equals, bit for bit, what the sequence call gives for the same CTU of the uncropped
 *      w x h picture: CTUs are independent everywhere except in the batch gates, whose 1024-CTU sub-batches are drawn over the picture's
 *      raster.  With closed gates, and w or h not a multiple of 64, the two may differ: replay is the cropped picture's result.
 *   Chunks: a run is replayed a chunk of frames at a time (ethcnn_replay_set_chunk_frames; 0 = default, 256 MB of residual planes).  The
 *      state goes from chunk to chunk by the sequence call's resident-state rule, so a chunked run equals an unchunked one bit for bit.
 *      The context's resident LDP state afterwards is the run's last.
 *   Memory of ethcnn_replay_run_device for a run of F frames in chunks of Fc: Fc nctu 4096 (one chunk's residual planes) + F nctu 8 (the
 *      run's source table) + F nctu 84 when d_probs is NULL + F nctu 16 when d_labels is NULL + nctu 3584 (the zero state) when f0 > 1
 *      + the copy of the records (n 16516) after ethcnn_replay_open_records.  ethcnn_replay_run_bytes returns that sum; it is held
 *      against max_bytes (0 = no limit of its own) and against the free device memory before anything is allocated, and
 *      ETHCNN_ERR_NOMEM carries it and leaves the object usable.  The buffers are kept until the next call that needs other sizes.
 *      Outside the sum: what the sequence call holds itself (ethcnn_ldp_sequence_bytes for nf = Fc), and 20 bytes a record of headers
 *      while ethcnn_replay_open_set runs.
 *   Errors: ETHCNN_ERR_NOWEIGHTS without a CNN or without an LSTM bundle; ETHCNN_ERR_FORMAT for an All-Intra set, a set that is not
 *      built, a byte count that is zero or not whole records, or an invalid run; ETHCNN_ERR_ARG for a bad run or slot, or when nothing is
 *      open.  Text: ethcnn_replay_last_error (ethcnn_last_error of the context for ethcnn_replay_create and
 *      ethcnn_replay_uncut_device). */
typedef struct ethcnn_replay ethcnn_replay;
typedef struct ethcnn_replay_run {
    int32_t seq, w, h;   /* the run's key: sequence number, width and height as in the headers */
    int32_t rows, cols;  /* R, C */
    uint32_t f0;         /* first frame number */
    int64_t frames;      /* F */
    int64_t nctu;        /* R C */
    int32_t qp[4];       /* slot QPs */
    int64_t src_offset;  /* first entry of the run in the table of ethcnn_replay_plan */
} ethcnn_replay_run;
/* The plan alone, on the host (no context, no GPU), over whole records.  runs_out (may be NULL) takes the first max_runs runs,
 * *nruns_out their total; src_out (may be NULL) holds nbytes / 16516 entries: the source tables of the runs back to back, run k from
 * src_offset on.  err (may be NULL) takes the text of ETHCNN_ERR_FORMAT. */
int ethcnn_replay_plan(const uint8_t* records, size_t nbytes, ethcnn_replay_run* runs_out, int max_runs, int* nruns_out, int64_t* src_out,
                       char* err, size_t errcap);
/* The kernel alone, on buffers in HBM; the counterpart of ethcnn_samples_cut_device.  d_src [nframes][R C] (8-byte aligned) picks records
 * of d_records (4-byte aligned, nrecords of them); d_resi [nframes][64 R][64 C] (16-byte aligned) and d_labels [nframes][4 R][4 C] (4-byte
 * aligned) are written, every byte once.  An index outside [0, nrecords) gives zeros.  Asynchronous on the context's stream. */
int ethcnn_replay_uncut_device(ethcnn_ctx* ctx, const uint8_t* d_records, int64_t nrecords, const int64_t* d_src, int64_t nframes, int R, int C,
                               int slot, uint8_t* d_resi, uint8_t* d_labels);
int ethcnn_replay_create(ethcnn_ctx* ctx, uint64_t max_bytes, ethcnn_replay** out);
void ethcnn_replay_destroy(ethcnn_replay* rp); /* before ethcnn_destroy of its context, and before the set it has open */
const char* ethcnn_replay_last_error(const ethcnn_replay* rp);
/* Opening replaces whatever was open.  A set (built, inter, of the same context) is only read and stays as it is; it must outlive its use
 * here.  Host records are planned on the host first (nothing is allocated for an invalid file), then uploaded in pieces of 64 MB. */
int ethcnn_replay_open_set(ethcnn_replay* rp, ethcnn_samples* inter_set);
int ethcnn_replay_open_records(ethcnn_replay* rp, const uint8_t* records, size_t nbytes);
int ethcnn_replay_run_count(const ethcnn_replay* rp);
int ethcnn_replay_run_info(ethcnn_replay* rp, int run, ethcnn_replay_run* out); /* src_offset: into the object's own table */
int ethcnn_replay_set_chunk_frames(ethcnn_replay* rp, int frames);
int64_t ethcnn_replay_run_bytes(ethcnn_replay* rp, int run, int own_probs, int own_labels); /* the memory sum above; negative: error */
/* Uncut, then the sequence call, chunk by chunk.  d_probs float32 [F][nctu][21] and d_labels uint8 [F][4 R][4 C] in HBM; either may be
 * NULL: the object's own buffer is used then.  Asynchronous on the context's stream. */
int ethcnn_replay_run_device(ethcnn_replay* rp, int run, int slot, float* d_probs, uint8_t* d_labels);
/* Several slots of a run through an ethcnn_ldp_group (config #5 offline, group form) of the same context: per chunk the uncut kernel runs
 * once per listed slot, then ONE group call runs on the chunk's planes with member j at slot slots[j] and that slot's QP; the bundle of
 * member j is the caller's choice, as the context's is for ethcnn_replay_run_device.  nslots must equal the group's member count; a slot
 * may be listed more than once.  d_probs[j] float32 [F][nctu][21] and d_labels[j] uint8 [F][4 R][4 C] in HBM, all given.  Per slot the
 * outputs equal ethcnn_replay_run_device(rp, run, slots[j], ...) on a context with member j's bundle, word for word; chunked equals
 * unchunked.  The states travel in the group's resident buffers; the context's resident LDP state stays as it is.
 * Memory: ethcnn_replay_run_group_bytes = nslots x Fc nctu 4096 (the chunk's planes of every slot) + F nctu 8 + nctu 3584 when f0 > 1
 * + the copy of the records; held against max_bytes and the free device memory as ethcnn_replay_run_bytes is.  Outside the sum: what
 * the group holds (ethcnn_ldp_group_bytes).  The object keeps its buffers at exactly the sizes of the last call: a caller that alternates
 * this entry and ethcnn_replay_run_device on one run frees and reallocates the plane buffer and waits for the stream at every switch
 * (the results are the same; replay one way, then the other).  Asynchronous on the context's stream. */
int64_t ethcnn_replay_run_group_bytes(ethcnn_replay* rp, int run, int nslots);
int ethcnn_replay_run_group_device(ethcnn_replay* rp, int run, int nslots, const int* slots, ethcnn_ldp_group* grp, float* const* d_probs,
                                   uint8_t* const* d_labels);
/* ethcnn_replay_run_device into the object's own buffers, then ethcnn_calib_add_frames_device / ethcnn_sim_add_frames_device with
 * width = 64 C, height = 64 R, skip_label_frames = 0: nothing goes through the host.  Synchronous, as those entries are. */
int ethcnn_replay_feed_calib(ethcnn_replay* rp, int run, int slot, ethcnn_calib* cal);
int ethcnn_replay_feed_sim(ethcnn_replay* rp, int run, int slot, ethcnn_sim* sim);
/* Several runs through an ethcnn_ldp_batch (config #5 offline, batch form) of the same context: item j = run runs[j] at slot slots[j]
 * with bundle bundles[j] of the batch, nitems = 1..32.  The runs may differ in geometry, length and first frame; a run may be listed more
 * than once, with different slots.  Per chunk the uncut kernel runs once per item that still has frames, then ONE batch call runs on
 * the chunk's planes.  Per item the outputs equal ethcnn_replay_run_device(rp, runs[j], slots[j], ...) on a context with that item's
 * bundle, word for word (the start state is zero, also when f0 > 1); chunked equals unchunked.  The chunk is Fc frames for all items:
 * ethcnn_replay_set_chunk_frames, else max(1, floor(256 MB / sum_j nctu_j 4096)).  The states travel in the batch's resident buffers
 * (the items are handed to the batch longest first, so the sequence indices they use are an implementation matter: do not mix these
 * entries with calls of ethcnn_ldp_batch_run_device that continue from resident states).
 * Memory: ethcnn_replay_batch_bytes = sum_j (min(F_j, Fc) nctu_j 4096 + F_j nctu_j 8) + 3584 x the largest nctu_j of the items with
 * f0 > 1 + the copy of the records; the feed entries hold sum_j F_j nctu_j (84 + 16) more for the object's own outputs.  What a call
 * holds is checked against max_bytes and the free device memory before anything is allocated.  Outside the sum: what the batch holds
 * (ethcnn_ldp_batch_bytes).  ethcnn_replay_batch_device: d_probs[j], d_labels[j] in HBM, all given; asynchronous on the context's stream.
 * The feed entries replay into the object's own buffers and then add the items to the consumer in list order with the arguments of
 * ethcnn_replay_feed_calib / _feed_sim: the consumer ends in exactly the state the per-run feeds in that order leave.  Synchronous.
 * Thresholds: ethcnn_replay_run_group_device and ethcnn_replay_batch_device use the group / batch as it is, every member or sequence
 * index under its resolved pair (ethcnn_ldp_set_thresholds_batch).  The feed entries need open gates: a batch in which ANY sequence index
 * holds a pair of its own is ETHCNN_ERR_ARG before anything is enqueued, and the text names the index. */
int64_t ethcnn_replay_batch_bytes(ethcnn_replay* rp, ethcnn_ldp_batch* b, int nitems, const int* runs);
int ethcnn_replay_batch_device(ethcnn_replay* rp, ethcnn_ldp_batch* b, int nitems, const int* runs, const int* slots, const int* bundles,
                               float* const* d_probs, uint8_t* const* d_labels);
int ethcnn_replay_batch_feed_calib(ethcnn_replay* rp, ethcnn_ldp_batch* b, int nitems, const int* runs, const int* slots, const int* bundles,
                                   ethcnn_calib* cal);
int ethcnn_replay_batch_feed_sim(ethcnn_replay* rp, ethcnn_ldp_batch* b, int nitems, const int* runs, const int* slots, const int* bundles,
                                 ethcnn_sim* sim);

#ifdef __cplusplus
}
#endif
#endif /* ETHCNN_H */
