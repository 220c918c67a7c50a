/*
 * wwhip.h - C ABI of libwwhip.so, the MI355X (gfx950) wake-word inference hot path.
 *
 * The reference (MerlinPCarson/WakeWord-Detection) has no FFI of its own: its hot path is
 * NumPy + the TensorFlow-Lite interpreter behind Python duck-typed classes.  Each entry
 * point below names the reference interface it replaces (paths relative to the reference
 * repository root).  The Python host classes in wakeword-detection_amd/wwhip/ bind these
 * with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every function returns 0 on success or a negative WW_E* code and never throws;
 *     ww_last_error(ctx) holds a human-readable message for the last failure on that ctx;
 *   - one ww_ctx per host thread; a ctx owns one HIP stream (or borrows the caller's) and a
 *     growable device workspace; calls on one ctx are serialised by the caller;
 *   - "host" entry points take ordinary host pointers, copy through pinned staging and
 *     return after the result is in the caller's buffer (PCIe inclusive);
 *   - "_dev" entry points take device pointers (e.g. torch tensor .data_ptr()), enqueue on
 *     the ctx stream and return without synchronising;
 *   - the caller owns every buffer it passes; nothing is retained after return except by
 *     ww_model_load (copies the blob) and the ww_streams object (owns its rings).
 */
#ifndef WWHIP_H
#define WWHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WW_OK 0
#define WW_EINVAL (-1)    /* bad argument (maps to ValueError) */
#define WW_EBLOB (-2)     /* malformed weight blob (ValueError) */
#define WW_EHIP (-3)      /* HIP runtime failure (RuntimeError) */
#define WW_ENOMEM (-4)    /* allocation failure (MemoryError) */
#define WW_ESTATE (-5)    /* object used in the wrong state (RuntimeError) */
#define WW_ENODEVICE (-6) /* no usable gfx950 device (RuntimeError) */
#define WW_EINTERNAL (-7) /* an exception stopped at the C boundary (RuntimeError); ww_last_error has its text */

#define WW_KIND_CRNN 1
#define WW_KIND_WAVENET 2

#define WW_FFT_WINDOW 512 /* (257 - 1) * 2, reference spokestack/wakeword/tflite.py:67 */
#define WW_FFT_BINS 257
#define WW_CHUNK 320 /* 20 ms @ 16 kHz, reference spokestack/io/pyaudio.py:24 */

typedef struct ww_ctx ww_ctx;
typedef struct ww_model ww_model;
typedef struct ww_streams ww_streams;

typedef struct ww_model_info {
  int32_t kind;      /* WW_KIND_* */
  int32_t window;    /* mel frames per inference: 151 (CRNN) / 182 (Wavenet) */
  int32_t n_mel;     /* 40 */
  int32_t n_bins;    /* 257 */
  int32_t n_out;     /* width of the detect output row: 1 (sigmoid) or 2 (softmax) */
  int32_t enc_rows;  /* encoder output rows: 1 (CRNN) / 182 (Wavenet) */
  int32_t enc_width; /* encoder output width: 64 (CRNN) / 32 (Wavenet) */
  int32_t reserved;
} ww_model_info;

/* Front-end parameters.  Reference: spokestack/wakeword/tflite.py:33-43,150-158 and
 * utils/tf_lite/filter.py:9-19,42-44. */
typedef struct ww_frontend_params {
  float pcm_divisor;  /* 32767 (streaming plugin, tflite.py:150) or 32768 (librosa floats) */
  int32_t clip;       /* 1: clip to [-1, 1] after the division (tflite.py:151) */
  float pre_emphasis; /* alpha of x[n] -= alpha * x[n-1]; reference default 0.0 */
  int32_t hop;        /* samples between frames: 160 (fft_hop_length 10 ms @ 16 kHz) */
  int32_t precise;    /* 1: Hann product + FFT in fp64 like the reference (tflite.py:175);
                         0: fp32 butterflies (faster, ~1e-6 relative on the magnitudes) */
} ww_frontend_params;

/* ---- context ------------------------------------------------------------------------- */
/* external_stream: NULL -> the ctx creates its own non-blocking stream; otherwise a
 * hipStream_t owned by the caller (e.g. torch.cuda.current_stream().cuda_stream). */
int ww_ctx_create(int device, void *external_stream, ww_ctx **out);
int ww_ctx_destroy(ww_ctx *ctx);
int ww_ctx_synchronize(ww_ctx *ctx);
void *ww_ctx_stream(ww_ctx *ctx);
/* ctx may be NULL: the error of the calling THREAD's last failed ww_ctx_create (thread-local text). */
const char *ww_last_error(const ww_ctx *ctx);
/* "wwhip <major>.<minor> (...; ABI <n>: ...)".  The ABI number changes whenever an existing entry point changes its
 * signature (ABI 4, round 4: ww_stream_create gained `flags` in round 3 - a host built against an older header must be
 * rebuilt); wwhip/_lib.py parses the number at load time and refuses a library of another ABI. */
#define WW_ABI 4
const char *ww_version(void);
/* Which HIP runtime the library actually runs on.  libwwhip.so links libamdhip64 by soname; a host program that has
 * already loaded another copy (PyTorch-ROCm wheels bundle their own) decides which one that is.  built_hip_version =
 * HIP_VERSION of the headers at compile time, runtime_version / driver_version = hipRuntimeGetVersion /
 * hipDriverGetVersion of the loaded runtime (0 if unavailable), all as major * 10,000,000 + minor * 100,000 + patch.
 * The Python binding warns when the major versions differ (wwhip/_lib.py). */
int ww_runtime_info(int32_t *built_hip_version, int32_t *runtime_version, int32_t *driver_version);

/* Host-side staging for the sharded evaluators (wwhip/evaluate.py; replaces the per-sample ring writes and pydub joins of
 * utils/evaluate_models.py:45-61,150-160 on the way to ONE upload): writes dst[0 .. total) once - run j copies count[j]
 * samples from src[j] to dst + dst_off[j] (runs disjoint, dst_off ascending), everything between the runs is zeroed (the
 * 0.5 s paddings and 100 ms gaps of the reference flow) - with `threads` host threads, each owning a contiguous slice of
 * dst.  No GPU call; dst is normally page-locked.  WW_EINVAL on overlapping or descending runs.  Only dst[lo .. hi) is
 * written (0 <= lo <= hi <= total): a caller stages a large buffer in a few slices and starts each slice's upload while the
 * next one is being written. */
int ww_host_stage_i16(int16_t *dst, int64_t total, int64_t n_runs, const int64_t *dst_off, const int16_t *const *src,
                      const int64_t *count, int64_t lo, int64_t hi, int32_t threads);

/* The same staging on a thread of the library's own, followed by the upload: an uploader owns `slots` page-locked buffers
 * (grown on demand), `copy_threads` copy threads and a copy stream on the context's device.  One submit = one chunk of a
 * rank's share of a test split: dst[0 .. total) assembled from the runs as ww_host_stage_i16 does, then copied to d_pcm, and
 * n_meta int64 words (the chunk's sample / frame offset tables) copied to d_meta.  The call copies the run arrays and `meta`
 * and returns at once with a ticket (1, 2, ...; chunks are processed in ticket order); the CLIP samples src[j] point to must
 * stay where they are until ww_uploader_wait(ticket) has returned.  ww_uploader_poll: 1 once the ticket's copies are enqueued,
 * 0 before.  ww_uploader_wait blocks the calling host thread until they are, then makes the context's stream wait for them
 * on the device (no host wait for the transfer itself) - the caller launches its kernels over d_pcm right behind it - and
 * reports what went wrong with the chunk if anything did (WW_EINVAL: overlapping runs; WW_ENOMEM; WW_EHIP).  Each ticket is
 * waited for at most once.  The reference has no counterpart: its evaluator feeds one wav at a time, 20 ms per step
 * (utils/evaluate_models.py:52-88); this is the transport that keeps two hours of audio per GPU moving while the interpreter
 * plans the next chunk.  One host thread drives an uploader; ww_uploader_destroy finishes what was submitted. */
typedef struct ww_uploader ww_uploader;
int ww_uploader_create(ww_ctx *ctx, int32_t slots, int32_t copy_threads, ww_uploader **out);
int ww_uploader_destroy(ww_uploader *up);
int ww_uploader_submit(ww_uploader *up, int64_t total, int64_t n_runs, const int64_t *dst_off, const int16_t *const *src,
                       const int64_t *count, int16_t *d_pcm, int64_t n_meta, const int64_t *meta, int64_t *d_meta, int64_t *ticket);
int ww_uploader_poll(ww_uploader *up, int64_t ticket);
int ww_uploader_wait(ww_uploader *up, int64_t ticket, ww_ctx *ctx);

/* Per-kernel timing with HIP events on the ctx stream (bench.py roofline leg).  While
 * enabled every kernel launch is bracketed by two events; ww_profile_read synchronises and
 * writes a JSON object {"kernel": {"calls": n, "total_ms": t}, ...}. */
int ww_profile_enable(ww_ctx *ctx, int on);
int ww_profile_read(ww_ctx *ctx, char *json, size_t cap);
/* Event pair on the ctx stream around an arbitrary region. */
int ww_timer_start(ww_ctx *ctx);
int ww_timer_stop(ww_ctx *ctx, float *elapsed_ms); /* synchronises on the stop event */

/* ---- model --------------------------------------------------------------------------- */
/* Replaces TFLiteModel.__init__ for the filter/encode/detect triple
 * (spokestack/models/tensorflow.py:24-31).  `blob` is the packed weight image produced by
 * wwhip.weights.pack_blob from the reference's .tflite files:
 *   u32 magic 'WWHB' | u32 version 1 | u32 kind | u32 n_sections
 *   n_sections x { char name[24]; u32 offset_bytes; u32 count }   then 16-byte aligned payload
 * Weights are uploaded once and stay resident in HBM.
 * Sections of a CRNN (float32 unless said otherwise; G = 3 gate blocks z, r, h for a reset-after GRU, G = 4 blocks i, f, c, o for an
 * LSTM; H units, F the width of the head's first layer):
 *   crnn.meta      int32[14]  n_mel, T, C, KF, KT, SF, ST, PF, PT, OF, OT, H, NOUT, HEAD
 *   crnn.cell      int32[2]   cell (WW_CELL_GRU | WW_CELL_LSTM), F.  OPTIONAL: absent means GRU and F = 2H, and pack_blob writes it
 *                             only for another cell or another F, so a blob of the shipped combination keeps its bytes.
 *   crnn.conv_w [C][KF][KT], crnn.conv_b [C]
 *   crnn.g{1,2}{f,b}.wx [G H][in], .bx [G H], .wh [G H][H], .bh [G H]   layer 1 | 2, forward | backward; in = OF C | 2H.
 *                             A GRU carries all four; an LSTM has ONE bias, .bx, and carries NO .bh section.
 *   crnn.head_w1 [F][2H], crnn.head_b1 [F]    (absent for WW_HEAD_CTC), crnn.head_w2 [NOUT][F], crnn.head_b2 [NOUT]
 * Accepted: H in {16, 32, 48, 64}, F in 1..64, either cell; refused with WW_EBLOB and a text naming the rule: an unknown cell, another
 * H or F, an LSTM blob with .bh, a GRU blob without, WW_HEAD_CTC on anything but GRU / H = 32.  Everything except (GRU, H = 32,
 * F = 64, the standard conv) runs the layered path of csrc/crnn.hip (conv_generic_kernel, gemm_nt_kernel, rnn_layer_kernel,
 * crnn_head_kernel). */
#define WW_CELL_GRU 0
#define WW_CELL_LSTM 1
int ww_model_load(ww_ctx *ctx, const void *blob, size_t len, ww_model **out);
int ww_model_free(ww_model *model);
int ww_model_get_info(const ww_model *model, ww_model_info *out);
/* The detect head of a CRNN (crnn.meta[13] of the blob); a Wavenet answers WW_HEAD_SOFTMAX, which is what its detect graph ends in.
 *   WW_HEAD_SIGMOID / WW_HEAD_SOFTMAX  Arik_CRNN (wwdetect/CRNN/model.py:21-56): Dense(64, relu) -> Dense(n_out) on the last states
 *   WW_HEAD_CTC                        Arik_CRNN_CTC (model.py:82-145): one Dense(n_out, softmax) on every step of layer 2, n_out =
 *                                      labels + blank.  Loaded only at the standard conv geometry, H = 32, 2 <= n_out <= 8; it
 *                                      runs through the ww_ctc_* family below and through nothing else (every other entry point
 *                                      that takes a model answers it with WW_EINVAL). */
#define WW_HEAD_SIGMOID 0
#define WW_HEAD_SOFTMAX 1
#define WW_HEAD_CTC 2
int ww_model_head_kind(const ww_model *model, int32_t *out);
/* The recurrent layers of a CRNN: cell (WW_CELL_GRU | WW_CELL_LSTM), units H per direction (the encoding is 2H wide) and head_units F
 * of the head's first dense layer.  WW_EINVAL for a Wavenet or a NULL pointer. */
int ww_model_rnn_kind(const ww_model *model, int32_t *cell, int32_t *units, int32_t *head_units);

/* Arithmetic of the model contractions.  The reference runs fp32 TFLite kernels; SURVEY 8(d) cfg 3 asks
 * for the Wavenet convs on bf16 MFMA with fp32 accumulate next to an fp32 parity mode.
 *   WW_PRECISION_FP32   (default) v_mfma_f32_16x16x4_f32 everywhere: bit for bit a k-ordered fp32 fmaf chain.
 *   WW_PRECISION_BF16X3 Wavenet's 24 gated blocks as split-bf16: x = hi + lo (two bf16), a*b =
 *                       ah*bh + ah*bl + al*bh on v_mfma_f32_16x16x32_bf16, fp32 accumulate; 16 mantissa
 *                       bits per operand - posteriors within 4e-6 of fp32 (tolerance 1e-4).  Plain
 *                       single-pass bf16 misses the tolerance (6e-4 .. 1e-3) and is not offered.
 *                       CRNN models: the conv and the layer-1 input projection (88 % of the FLOPs) take the same
 *                       split form (crnn_fused_bf16_kernel); the recurrences and the head stay fp32; posteriors
 *                       within 1e-5 of fp32.  (CRNNs of another conv geometry keep fp32.)
 * (Value 2 was round 1's experimental BF16X6 projection mode; it was not faster than fp32 and is retired: WW_EINVAL.) */
#define WW_PRECISION_FP32 0
#define WW_PRECISION_BF16X3 1
int ww_model_set_precision(ww_model *model, int precision);

/* Dispatch options of one model object (they select between kernels that compute the same windows; results agree to
 * <= 2e-6, tests/test_gpu_parity.py).  These replace round 2's process-wide WWHIP_CRNN_* environment variables.
 *   WW_OPT_CRNN_SPLIT_AT   explicit-window launches above this many windows run crnn_fused_kernel<front> + gru_tail_kernel
 *                          instead of one crnn_fused_kernel (default 1024; 0 = always one fused kernel)
 *   WW_OPT_CRNN_SLIDE_MIN  regular sliding windows (ww_slide_forward, ww_forward_segments_dev) take the once-per-sequence
 *                          form crnn_rows_kernel + gru_tail_kernel from this many windows on (default 64; 0 = never)
 *   WW_OPT_CRNN_TAIL_MFMA  the recurrences of those two forms: sixteen windows per workgroup with the recurrent products and
 *                          the layer-2 projection on v_mfma_f32_16x16x4_f32 (gru_tail16_kernel), or one window per workgroup
 *                          on the vector ALU (gru_tail_kernel).  1 (default) = the matrix form from 9,216 windows per launch on
 *                          (below that its 38-step serial chain on few workgroups loses); 2 = always; 0 = never; any other
 *                          value: WW_EINVAL
 *   WW_OPT_WAVENET_ROWMAJOR 0 (default) = the fp32 Wavenet block loop in transposed form (channels x time: BatchNorm output and
 *                          gate product feed the next MFMA straight from registers); 1 = rounds 1-2's row-major loop (both
 *                          through LDS).  Same products, another summation order of the three taps and the bias. */
#define WW_OPT_CRNN_SPLIT_AT 1
#define WW_OPT_CRNN_SLIDE_MIN 2
#define WW_OPT_CRNN_TAIL_MFMA 3
#define WW_OPT_WAVENET_ROWMAJOR 4
/*   WW_OPT_WAVE_SEQ_SEGMENT rows per independently computed segment of the Wavenet's sequence form (ww_wave_sequence); 0 (default) = the
 *                          library's choice.  Every value gives the same bits: it exists so that a test can move the cuts. */
#define WW_OPT_WAVE_SEQ_SEGMENT 5
int ww_model_set_option(ww_model *model, int key, int64_t value);

/* ---- model sets: several models of ONE geometry behind one launch and one stream bank -----------
 * The reference evaluates lists of checkpoints over the same audio (wwdetect/wavenet/evaluate_wavenet.py: eval_models; utils/
 * plot_eval_models.py) one TFLite interpreter at a time, and a service holds one wake word per tenant.  A loaded model is one
 * device block whose layout depends on its geometry alone, so K models of one geometry are K blocks at a fixed stride:
 * ww_model_set_create copies the members' blocks, device to device on the context's stream, into ONE allocation of n_models x stride
 * (stride = the block size rounded up to 256 bytes), and the kernels add member x stride to their weight pointers, once per
 * workgroup.  The members may be freed afterwards; the set must outlive the banks created from it.  Member k evaluated through a set
 * gives the bits member k gives on its own.  ONE front end serves the set.
 * WW_EINVAL (ww_last_error says which member and why): n_models outside 1..WW_SET_MAX_MODELS or NULL arguments; a member of another
 * context; members of different kind, or whose ww_model_info differs in any field; members whose geometry differs (a Wavenet's
 * dilations, block order and residual convs included) or is a CRNN's generic conv geometry; members whose block sizes differ; a
 * member in WW_PRECISION_BF16X3 (sets are fp32 only); members whose filters (filter.tflite: geometry and every array) are not
 * byte-identical.  ww_model_set_info: the members' common info and their number (either may be NULL). */
typedef struct ww_model_set ww_model_set;
#define WW_SET_MAX_MODELS 64
int ww_model_set_create(ww_ctx *ctx, const ww_model *const *models, int32_t n_models, ww_model_set **out);
int ww_model_set_destroy(ww_model_set *set);
int ww_model_set_info(const ww_model_set *set, ww_model_info *info, int32_t *n_models);

/* ---- front end: PCM -> log-mel ---------------------------------------------------------
 * Replaces the per-sample RingBuffer loop + np.fft.rfft + filter.tflite invoke of
 * Filter.filter_frame / WakewordTrigger._sample/_analyze/_filter
 * (utils/tf_lite/filter.py:38-75, spokestack/wakeword/tflite.py:148-191).
 *
 * Utterance u occupies samples [sample_offs[u], sample_offs[u+1]) of `pcm` and yields
 * nf(u) = max(0, (len - 512) / hop + 1) frames; frame j covers samples [hop*j, hop*j+512).
 * Row frame_offs[u] + j of `mel` receives its 40 log-mel values.  frame_offs (n_utt+1
 * entries) is written by the host variants and read by the device variants. */
int64_t ww_num_frames(int64_t n_samples, int32_t hop);

int ww_logmel(ww_ctx *ctx, const ww_model *model, const int16_t *pcm, const int64_t *sample_offs, int32_t n_utt,
              const ww_frontend_params *fp, float *mel, int64_t *frame_offs);
/* Same, for float samples already scaled to [-1, 1] (the offline path hands librosa floats
 * to Filter.filter_frame: utils/evaluate_models.py:46,64).  pcm_divisor / clip are ignored. */
int ww_logmel_f32(ww_ctx *ctx, const ww_model *model, const float *samples, const int64_t *sample_offs,
                  int32_t n_utt, const ww_frontend_params *fp, float *mel, int64_t *frame_offs);
/* STFT magnitudes only: frames [n][512] fp32 -> mag [n][257] fp32
 * (WakewordTrigger._analyze, spokestack/wakeword/tflite.py:174-176). */
int ww_stft_mag(ww_ctx *ctx, const ww_model *model, const float *frames, int64_t n, int32_t precise, float *mag);

/* filter.tflite on its own: mag [n][257] fp32 -> log-mel [n][40]  (TFLiteModel("filter.tflite")(frame),
 * spokestack/wakeword/tflite.py:183-184; utils/tf_lite/filter.py:72-73). */
int ww_filter_apply(ww_ctx *ctx, const ww_model *model, const float *mag, int64_t n, float *mel);

/* Device form of ww_logmel: the row of frame j of utterance u is the bits of the host form's.  Extent: samples outside
 * [d_sample_offs[0], d_sample_offs[n_utt]) never reach a row, a frame reads its own utterance only, and rows [0, total_frames) of
 * d_mel are written and nothing else. */
int ww_logmel_dev(ww_ctx *ctx, const ww_model *model, const int16_t *d_pcm, const int64_t *d_sample_offs,
                  const int64_t *d_frame_offs, int32_t n_utt, int64_t total_frames, int64_t max_frames_per_utt,
                  const ww_frontend_params *fp, float *d_mel);

/* ---- sample-rate conversion: audio at any rate -> the models' 16 kHz --------------------------
 * Stands where the reference's entry points call librosa.load(path, sr=16000) (utils/evaluate_models.py:46,
 * utils/filter_dataset_to_h5.py:70).  NOT librosa's bits: librosa's filters (soxr_hq, kaiser_best) are third-party code; the
 * transform here is the float64 statement below (wwhip/resample.py: design), evaluated in fp32.
 *   g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g, L = rate_in * up
 *   f2 = rolloff * min(rate_in, rate_out) / L, half = ceil(zeros / f2)
 *   h[i] = up * f2 * sinc(f2 * i) * kaiser(2 * half + 1, beta)[i + half], i = -half .. half  (np.sinc, np.kaiser, float64)
 *   y[m] = sum over k with |m * down - k * up| <= half of h[m * down - k * up] * x[k],  m = 0 .. ceil(n * up / down) - 1
 * which is scipy.signal.resample_poly(x, up, down, window=h / up).  x reads as zero outside its signal; int16 input is scaled
 * by exactly 1 / 32768.  taps per output = ceil((2 * half + 1) / up).  rate_in == rate_out: no filter, y = x bit for bit.
 * Arithmetic: y[m] is ONE fp32 fmaf chain from 0 over its input samples in ascending k, taps rounded once from float64 - its
 * bits depend on m, the filter and the samples of its span only, not on tiles, batch neighbours or how a stream was cut.
 * params == NULL: zeros 32, rolloff 0.945, beta 14.769656459379492. */
typedef struct ww_resampler ww_resampler;
typedef struct ww_resampler_params {
  double rolloff, beta;
  int32_t zeros, reserved;
} ww_resampler_params;
typedef struct ww_resample_info {
  int64_t up, down, half, taps_per_output, table_bytes; /* table_bytes: the fp32 tap table on the device */
} ww_resample_info;
/* A filter whose table (up * taps per output) exceeds WW_RESAMPLE_MAX_TAPS, or whose tile (2 * down + taps per output + 2
 * staged samples) exceeds WW_RESAMPLE_MAX_SPAN, is refused with WW_EINVAL: every pair of the standard rates 8, 11.025, 16,
 * 22.05, 24, 32, 44.1, 48, 88.2, 96, 176.4, 192 kHz passes (largest table: 11.025 kHz -> 192 kHz, 174,080 taps; 192 kHz ->
 * 11.025 kHz has 173,460 and the longest tile, 2 * 2560 + 1180 + 2 staged samples), 44101 <-> 16000 (2.99 M taps) does not.
 * Rates <= 0: WW_EINVAL. */
#define WW_RESAMPLE_MAX_TAPS (1 << 20)
#define WW_RESAMPLE_MAX_SPAN 12288
#define WW_SAMPLE_I16 0
#define WW_SAMPLE_F32 1
/* G.711 (ITU-T), one byte per sample, as a telephony leg carries it: an INPUT format of ww_resample / ww_resample_dev (and of the
 * stream banks' formats below).  A code decodes to the 16-bit sample audioop.ulaw2lin(b, 2) / audioop.alaw2lin(b, 2) give:
 *   mu-law:  v = ~code & 0xFF;  t = (((v & 0x0F) << 3) + 0x84) << ((v & 0x70) >> 4);  x = (v & 0x80) ? 0x84 - t : t - 0x84
 *   A-law:   v = code ^ 0x55;   t = (v & 0x0F) << 4;  seg = (v & 0x70) >> 4;
 *            seg == 0 ? t += 8 : (t += 0x108, t <<= seg - 1);  x = (v & 0x80) ? t : -t
 * (mu-law: +-32124, 255 distinct values; A-law: +-32256, 256 distinct values.)  The codes are decoded in the kernels that read the
 * samples, and A G.711 INPUT YIELDS THE BITS THE SAME CALL YIELDS ON THE DECODED int16 SAMPLES - no tolerance.  Samples are one byte
 * each: sample_offs counts samples as ever, and a segment may start at any byte.  As out_format they are WW_EINVAL.  rate_in ==
 * rate_out: the output is the decoded signal (WW_SAMPLE_I16: exactly; WW_SAMPLE_F32: times 2^-15).  (Value 2 is no format.)
 * ww_g711_table writes the 256 decoded values of WW_SAMPLE_MULAW or WW_SAMPLE_ALAW; host only, no context; another format, or a NULL
 * table, is WW_EINVAL. */
#define WW_SAMPLE_MULAW 8
#define WW_SAMPLE_ALAW 9
int ww_g711_table(int32_t format, int16_t table[256]);
int ww_resampler_create(ww_ctx *ctx, int32_t rate_in, int32_t rate_out, const ww_resampler_params *params, ww_resampler **out);
int ww_resampler_destroy(ww_resampler *r);
int ww_resampler_info(const ww_resampler *r, ww_resample_info *out);
/* Output ranges of n_seg segments in one launch.  Segment u holds samples [sample_offs[u], sample_offs[u + 1]) of `in`
 * (WW_SAMPLE_I16, WW_SAMPLE_F32, WW_SAMPLE_MULAW or WW_SAMPLE_ALAW), which are samples in_first[u] .. of its own signal; outputs out_first[u] .. of that signal,
 * out_offs[u + 1] - out_offs[u] of them, go to out[out_offs[u] .. out_offs[u + 1]) as WW_SAMPLE_F32, or as WW_SAMPLE_I16 =
 * clip(rint(y * 32768), -32768, 32767).  Samples outside a segment read as zero.  in_first / out_first == NULL: all zero (a
 * one-shot clip: count = ceil(n * up / down)).  A long signal in pieces, or a stream in packets: give each piece
 * ceil(half / up) samples of history in front of the first sample its outputs need - the pieces are the one-shot's bits.
 * All offset arrays are HOST arrays, consumed before the call returns.  WW_EINVAL (nothing is written): n_seg < 0, NULL where
 * data is needed, an unknown format, negative or descending offsets, an output range beyond ceil((in_first + n) * up / down).
 * n_seg = 0 and empty segments are WW_OK and write nothing.  ww_resample takes host pointers and returns with the result in
 * `out`; ww_resample_dev takes device pointers, enqueues on the context's stream and does not synchronise. */
int ww_resample(ww_resampler *r, const void *in, int32_t in_format, const int64_t *sample_offs, const int64_t *in_first,
                const int64_t *out_first, const int64_t *out_offs, int32_t n_seg, void *out, int32_t out_format);
int ww_resample_dev(ww_resampler *r, const void *d_in, int32_t in_format, const int64_t *sample_offs, const int64_t *in_first,
                    const int64_t *out_first, const int64_t *out_offs, int32_t n_seg, void *d_out, int32_t out_format);

/* ---- encode + detect -------------------------------------------------------------------
 * Replaces encode_model(x) followed by detect_model(x) (two TFLiteModel.__call__,
 * spokestack/wakeword/tflite.py:193-231; utils/evaluate_models.py:76-86;
 * utils/evaluate_tf_lite_opts.py:49-69).  `windows` is [B][window][n_mel] fp32, rows in
 * time order exactly as RingBuffer.read_all returns them (the CRNN transpose to
 * [1,40,151,1] of tflite.py:199-203 is folded into the kernel's indexing).
 * `out` receives [B][n_out]: the detect graph's output row. */
int ww_forward(ww_ctx *ctx, const ww_model *model, const float *windows, int32_t n_windows, float *out);
/* Optional: also return the encoder output ([B][enc_rows][enc_width]); enc may be NULL. */
int ww_forward_enc(ww_ctx *ctx, const ww_model *model, const float *windows, int32_t n_windows, float *out,
                   float *enc);

/* detect.tflite on its own: encoder outputs [n][enc_rows][enc_width] -> detect rows [n][n_out]
 * (TFLiteModel("detect.tflite")(x), spokestack/wakeword/tflite.py:228-231). */
int ww_detect(ww_ctx *ctx, const ww_model *model, const float *enc, int32_t n, float *out);

/* Sliding evaluation of one mel sequence (utils/evaluate_models.py:66-88): window i covers
 * rows [i*hop, i*hop + window); n_windows = (rows - window) / hop + 1 (0 if rows < window).
 * The windows are never materialised: kernels index the sequence directly. */
int ww_slide_forward(ww_ctx *ctx, const ww_model *model, const float *mel, int64_t rows, int32_t hop, float *out,
                     int64_t *n_windows);

/* Device form.  Window w reads mel rows [d_win_row[w], d_win_row[w] + d_win_valid[w]) and is
 * zero padded at the end up to `window` rows (evaluate_tf_lite_opts.py:43-45).
 * Extent: rows that no window names - the rows from d_win_valid[w] on, the rows between the windows - never reach a result, whatever
 * they hold (NaN and Inf included); d_out[0 .. n_windows) is written and nothing else; a non-finite value in a window's own rows
 * affects that window's row alone (tests/test_gpu_extents.py holds this for every _dev entry point that says "Extent"). */
int ww_forward_windows_dev(ww_ctx *ctx, const ww_model *model, const float *d_mel, int64_t mel_rows,
                           const int64_t *d_win_row, const int32_t *d_win_valid, int32_t n_windows, float *d_out);

/* ---- CTC-trained CRNNs (WW_HEAD_CTC): per-step label posteriors and their greedy decode --------------------------------------
 * What wwdetect/CRNN/evaluate.py:100-150 (eval_CTC) does with model.predict + K.ctc_decode(greedy=True): a window gives
 * T' = 19 rows of L posteriors (L = n_out = labels + blank, the blank is class L - 1; dataloader.py:54-62), and its decoded string is,
 * step by step, the argmax over the classes (lowest index on a tie), kept when it is not the blank and differs from the previous
 * step's argmax (the blank counts as a previous value: a, blank, a reads "a a").
 *   labels  [n][max_labels] int32: the first max_labels decoded labels, padded with -1;  1 <= max_labels <= 19
 *   lengths [n] int32: the whole decoded length (it may exceed max_labels)
 *   steps   [n][19][L] the posteriors, optional (NULL);  enc [n][19][64] layer 2's step outputs [h_fwd(t) | h_bwd(t)], optional
 * The decode reads the float32 posteriors as written to `steps`.  (Keras' ctc_decode takes log(y + 1e-7) first: monotone, so it can
 * only turn a strict order of two posteriors into a tie where they round together; the library decodes the posteriors themselves.)
 * fp32, standard conv geometry, one model: WW_EINVAL (before anything is written) for a model whose head is not WW_HEAD_CTC, a CTC
 * model in WW_PRECISION_BF16X3, a NULL required pointer, max_labels outside 1..19.  n = 0: WW_OK, nothing written.
 * Always crnn_fused_kernel<front>, then gru_tail_ctc_kernel (csrc/crnn.hip). */
int ww_ctc_forward(ww_ctx *ctx, const ww_model *model, const float *windows, int32_t n, int32_t max_labels, int32_t *labels,
                   int32_t *lengths, float *steps, float *enc);
/* Device form with ww_forward_windows_dev's windows: window w reads d_win_valid[w] rows from row d_win_row[w] and is zero padded at
 * the end - the dataloader's truncate-and-pad of a clip (wwdetect/CRNN/dataloader.py:90-92).  Extent: as ww_forward_windows_dev, for
 * each of the four outputs - rows [0, n) of each are written, and a window's non-finite rows reach that window's rows alone. */
int ww_ctc_forward_windows_dev(ww_ctx *ctx, const ww_model *model, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                               const int32_t *d_win_valid, int32_t n, int32_t max_labels, int32_t *d_labels, int32_t *d_lengths,
                               float *d_steps, float *d_enc);
/* Windows sliding over one mel sequence as in ww_slide_forward (*n_windows of them; labels / lengths / steps sized for that many).
 * WW_OPT_CRNN_SLIDE_MIN does not apply: crnn_rows_kernel's projected rows differ from the front kernel's in their last bits, and a
 * window's outputs here are the same bits whether it arrives under a hop or cut out and handed to ww_ctc_forward. */
int ww_ctc_slide_forward(ww_ctx *ctx, const ww_model *model, const float *mel, int64_t rows, int32_t hop, int32_t max_labels,
                         int32_t *labels, int32_t *lengths, float *steps, int64_t *n_windows);
/* The decode alone, on any device posteriors [n][T][L], 1 <= T <= 4096, 2 <= L <= 64 (csrc/ctc_decode.h's function, one thread per
 * row of the batch); labels / lengths as above with 1 <= max_labels <= T. */
int ww_ctc_greedy_dev(ww_ctx *ctx, const float *d_steps, int64_t n, int32_t T, int32_t L, int32_t max_labels, int32_t *d_labels,
                      int32_t *d_lengths);

/* ---- CTC-trained CRNNs: a wake-word SCORE from the forward algorithm ---------------------------------------------------------------
 * The reference trains these models with K.ctc_batch_cost against [HEY][SNIPS] (wwdetect/CRNN/train.py:184-200): -log of the
 * probability that a window's label sequence collapses to the target.  Evaluated at inference that probability is a number to put a
 * threshold on - what ww_far_frr[_dev], ww_posterior_events[_dev] and a stream bank's trigger need, and the greedy decode cannot give.
 * The statement, its recurrence and its arithmetic: csrc/ctc_score.h (wwhip.ctc.score is the same in float64).
 *   y [T][L] posteriors, the blank is class L - 1;  1 <= T <= 64 (the linear domain, no rescaling), 2 <= L <= 64
 *   targets [K][WW_CTC_SCORE_MAX_TARGET] int32 on the HOST, target_lens [K]: 1 <= K <= WW_CTC_SCORE_MAX_TARGETS targets of
 *     1 <= U <= WW_CTC_SCORE_MAX_TARGET labels in [0, L - 2], repeats allowed
 *   mode  WW_CTC_SCORE_EXACT   P(decode == target), the loss's quantity
 *         WW_CTC_SCORE_PREFIX  P(decode starts with target), the quantity of the trigger rule (ww_ctc_trigger_bank_step)
 *   score [K][n] float32, plane-major: plane k is a posterior track that ww_far_frr_dev / ww_posterior_events_dev take as it is
 * Every + and * is one float32 operation in the header's order, on the device and on the host: ww_ctc_score_dev gives the bits of
 * ww_ctc_score_rows.  Against the float64 statement on the same float32 posteriors the relative error is at most (3T + 2) 2^-24, plus
 * (2U + 1) T 2^-126 where values under FLT_MIN are flushed.  The posteriors themselves are read (Keras' loss renormalises
 * log(y + 1e-7) with a second softmax; the library does not copy that).
 * WW_EINVAL before anything is written, the text naming the rule: T outside 1..64, L outside 2..64, K or a target's length out of
 * range, a label outside [0, L - 2], an unknown mode, a NULL required pointer; the model forms also for a model that is not
 * WW_HEAD_CTC or is in WW_PRECISION_BF16X3, and for labels without lengths.  n = 0: WW_OK, nothing written.
 * ww_ctc_score_dev - ctc_score_kernel alone (csrc/ctc_score.hip) on any device posteriors [n][T][L]; rows [0, n) of each of the K
 *   planes are written, and a sequence's non-finite posteriors reach its own K scores alone.  Enqueued on the context's stream.
 * ww_ctc_score_rows - host only, no context (its refusal's text: ww_last_error(NULL)): the header's function over host arrays.
 * ww_ctc_score / _windows_dev / ww_ctc_slide_score - ww_ctc_forward / _windows_dev / ww_ctc_slide_forward with the score kernel behind
 *   every chunk's model launch, on the posteriors that ww_ctc_forward would return as `steps` (T = 19, L = n_out; they stay in the
 *   workspace).  labels [n][max_labels] and lengths [n] are optional, both or neither: the greedy decode beside the score. */
#define WW_CTC_SCORE_MAX_TARGET 9
#define WW_CTC_SCORE_MAX_TARGETS 8
#define WW_CTC_SCORE_EXACT 0
#define WW_CTC_SCORE_PREFIX 1
int ww_ctc_score_dev(ww_ctx *ctx, const float *d_steps, int64_t n, int32_t T, int32_t L, const int32_t *targets, const int32_t *target_lens,
                     int32_t K, int32_t mode, float *d_score);
int ww_ctc_score_rows(const float *steps, int64_t n, int32_t T, int32_t L, const int32_t *targets, const int32_t *target_lens, int32_t K,
                      int32_t mode, float *score);
int ww_ctc_score(ww_ctx *ctx, const ww_model *model, const float *windows, int32_t n, const int32_t *targets, const int32_t *target_lens,
                 int32_t K, int32_t mode, float *score, int32_t max_labels, int32_t *labels, int32_t *lengths);
int ww_ctc_score_windows_dev(ww_ctx *ctx, const ww_model *model, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                             const int32_t *d_win_valid, int32_t n, const int32_t *targets, const int32_t *target_lens, int32_t K,
                             int32_t mode, float *d_score, int32_t max_labels, int32_t *d_labels, int32_t *d_lengths);
int ww_ctc_slide_score(ww_ctx *ctx, const ww_model *model, const float *mel, int64_t rows, int32_t hop, const int32_t *targets,
                       const int32_t *target_lens, int32_t K, int32_t mode, float *score, int32_t max_labels, int32_t *labels,
                       int32_t *lengths, int64_t *n_windows);

/* ---- CTC-trained CRNNs: WHERE in a window the target lies (Viterbi alignment) ---------------------------------------------------------
 * The decode, the tick and the score say whether a window holds [HEY][SNIPS]; the stage behind the wake word (an activation timeout,
 * a recogniser fed the audio after the word) needs where.  The most probable path through the target's CTC lattice - the max-product
 * twin of the score's sum - and the steps at which it enters and leaves each label, to one conv step (80 ms at the standard
 * geometry; wwhip.ctc.step_rows maps a step to mel rows).  The statement, its tie rules and its arithmetic: csrc/ctc_align.h
 * (wwhip.ctc.align is the same in float64).  Arguments and limits are ww_ctc_score_*'s: y [T][L], targets [K][9], target_lens [K], mode
 *   WW_CTC_SCORE_EXACT   the best path whose collapse IS the target; it ends at step T - 1
 *   WW_CTC_SCORE_PREFIX  the best path up to the step t* at which it completes the target (what follows is free: the trigger's rule)
 *   value [K][n] float32: the probability of that path (one float32 multiplication per step)
 *   span  [K][n][WW_CTC_SCORE_MAX_TARGET][2] int8: {first step, last step} of label u on that path; in prefix mode the last label's
 *     pair is {t*, t*}; rows u >= U are -1; value == 0 (T too short, a zero posterior on every path, underflow): every row is -1
 * All K n values and all K n 18 span bytes are written.  On the device and on the host the same comparisons and multiplications in
 * the same order: ww_ctc_align_dev gives the bits of ww_ctc_align_rows.  Against the float64 statement on the same float32
 * posteriors the value is within (T - 1) 2^-24 relative (plus flushing under FLT_MIN), and the path is an optimal one up to twice that.
 * WW_EINVAL before anything is written, the text naming the rule: ww_ctc_score_*'s rules, and a NULL value or span.  n = 0: WW_OK.
 * ww_ctc_align_dev - ctc_align_kernel alone (csrc/ctc_align.hip) on any device posteriors [n][T][L], enqueued on the context's stream.
 * ww_ctc_align_rows - host only, no context (its refusal's text: ww_last_error(NULL)).
 * ww_ctc_align / _windows_dev / ww_ctc_slide_align - ww_ctc_score / _windows_dev / ww_ctc_slide_score with the align kernel in the
 *   score kernel's place behind every chunk's model launch; labels / lengths are the optional decode, as there. */
int ww_ctc_align_dev(ww_ctx *ctx, const float *d_steps, int64_t n, int32_t T, int32_t L, const int32_t *targets, const int32_t *target_lens,
                     int32_t K, int32_t mode, float *d_value, int8_t *d_span);
int ww_ctc_align_rows(const float *steps, int64_t n, int32_t T, int32_t L, const int32_t *targets, const int32_t *target_lens, int32_t K,
                      int32_t mode, float *value, int8_t *span);
int ww_ctc_align(ww_ctx *ctx, const ww_model *model, const float *windows, int32_t n, const int32_t *targets, const int32_t *target_lens,
                 int32_t K, int32_t mode, float *value, int8_t *span, int32_t max_labels, int32_t *labels, int32_t *lengths);
int ww_ctc_align_windows_dev(ww_ctx *ctx, const ww_model *model, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                             const int32_t *d_win_valid, int32_t n, const int32_t *targets, const int32_t *target_lens, int32_t K,
                             int32_t mode, float *d_value, int8_t *d_span, int32_t max_labels, int32_t *d_labels, int32_t *d_lengths);
int ww_ctc_slide_align(ww_ctx *ctx, const ww_model *model, const float *mel, int64_t rows, int32_t hop, const int32_t *targets,
                       const int32_t *target_lens, int32_t K, int32_t mode, float *value, int8_t *span, int32_t max_labels, int32_t *labels,
                       int32_t *lengths, int64_t *n_windows);

/* ---- CTC-trained CRNNs: prefix BEAM SEARCH, the n most probable label strings -----------------------------------------------------------
 * The greedy decode collapses the most probable path; it does not find the most probable label STRING, and ww_ctc_score_* needs its
 * targets named in advance.  The beam search gives the P most probable strings of a window with their probabilities - what
 * K.ctc_decode(greedy=False, beam_width, top_paths) is asked for.  The statement, its order and its arithmetic: csrc/ctc_beam.h
 * (wwhip.ctc.beam_search is the same in float64): the textbook prefix search on the posteriors themselves, in the linear domain.  It
 * is not a bit copy of TensorFlow's decoder, which works on log(y + 1e-7) in the log domain; the parity target is the float64 statement.
 *   y [T][L] posteriors, the blank is class L - 1;  1 <= T <= WW_CTC_BEAM_MAX_T, 2 <= L <= 8
 *   1 <= beam_width <= WW_CTC_BEAM_MAX_WIDTH, 1 <= top_paths <= min(beam_width, WW_CTC_BEAM_MAX_PATHS), 1 <= max_labels <= T
 *   labels  [n][top_paths][max_labels] int32: the first max_labels labels of path p, padded with -1
 *   lengths [n][top_paths] int32: the WHOLE length of path p (it may exceed max_labels; 0 is the empty string)
 *   prob    [n][top_paths] float32: P(decode == that string) as far as the beam saw it, descending (ties: shorter, then lexicographic)
 *   a path whose probability is 0, or that the beam has no entry for, is absent: length -1, every label -1, prob 0
 * Every + and * is one float32 operation in the header's order, every comparison the header's, on the device and on the host:
 * ww_ctc_beam_dev gives the bits of ww_ctc_beam_rows.  Against the float64 statement on the same float32 posteriors with the same
 * pruning decisions a probability is within (3T + 2) 2^-24 relative (derived in the header), plus 5 T (T + 1) 2^-126 where values
 * under FLT_MIN are flushed.
 * WW_EINVAL before anything is written, the text naming the rule: T, L, beam_width, top_paths or max_labels out of range, a NULL
 * required pointer; the model forms also for a model that is not WW_HEAD_CTC or is in WW_PRECISION_BF16X3.  n = 0: WW_OK, nothing
 * written.
 * ww_ctc_beam_dev - ctc_beam_kernel alone (csrc/ctc_beam.hip: a wave per sequence, a beam slot per lane) on any device posteriors
 *   [n][T][L]; rows [0, n) of each output are written and nothing else, and a sequence's non-finite posteriors reach its own outputs
 *   alone.  Enqueued on the context's stream, no synchronisation.
 * ww_ctc_beam_rows - host only, no context (its refusal's text: ww_last_error(NULL)): the header's function over host arrays.
 * ww_ctc_beam / _windows_dev / ww_ctc_slide_beam - ww_ctc_forward / _windows_dev / ww_ctc_slide_forward with the beam kernel behind
 *   every chunk's model launch, on the posteriors that ww_ctc_forward would return as `steps` (T = 19, L = n_out; they stay in the
 *   workspace).  The greedy decode is not carried beside it. */
#define WW_CTC_BEAM_MAX_T 19
#define WW_CTC_BEAM_MAX_WIDTH 64
#define WW_CTC_BEAM_MAX_PATHS 8
int ww_ctc_beam_dev(ww_ctx *ctx, const float *d_steps, int64_t n, int32_t T, int32_t L, int32_t beam_width, int32_t top_paths,
                    int32_t max_labels, int32_t *d_labels, int32_t *d_lengths, float *d_prob);
int ww_ctc_beam_rows(const float *steps, int64_t n, int32_t T, int32_t L, int32_t beam_width, int32_t top_paths, int32_t max_labels,
                     int32_t *labels, int32_t *lengths, float *prob);
int ww_ctc_beam(ww_ctx *ctx, const ww_model *model, const float *windows, int32_t n, int32_t beam_width, int32_t top_paths,
                int32_t max_labels, int32_t *labels, int32_t *lengths, float *prob);
int ww_ctc_beam_windows_dev(ww_ctx *ctx, const ww_model *model, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                            const int32_t *d_win_valid, int32_t n, int32_t beam_width, int32_t top_paths, int32_t max_labels,
                            int32_t *d_labels, int32_t *d_lengths, float *d_prob);
int ww_ctc_slide_beam(ww_ctx *ctx, const ww_model *model, const float *mel, int64_t rows, int32_t hop, int32_t beam_width,
                      int32_t top_paths, int32_t max_labels, int32_t *labels, int32_t *lengths, float *prob, int64_t *n_windows);

/* ---- CTC-trained CRNNs: HOW MUCH of each step belongs to each label (forward-backward occupancy) --------------------------------------
 * The alignment gives the one best path; this is the posterior over ALL the paths that read the target: given that the window reads
 * it, the share of step t that label u holds - the soft counterpart of the span, with the confidence of a boundary in it -, in
 * prefix mode the distribution of the step that completes the wake word, and in exact mode the per-class share whose difference from
 * the posteriors is the gradient of the CTC loss (-log of ww_ctc_score_*'s exact score) with respect to a step's logits.  The
 * statement and its arithmetic: csrc/ctc_occupancy.h (wwhip.ctc.occupancy is the same in float64).  Arguments and limits are
 * ww_ctc_score_*'s: y [T][L], targets [K][9], target_lens [K], mode
 *   value [K][n] float32: Z, the bits of ww_ctc_score_* for the same mode
 *   occ   [K][n][T][WW_CTC_SCORE_MAX_TARGET] float32: occ[t][u] = P(the path is on label u at step t | the target); in prefix mode
 *     u = U - 1 holds P(the target is completed at step t | it is completed), which sums to 1 over t; rows u >= U are +0
 *   cls   [K][n][T][L] float32, or NULL; exact mode only: the same posterior per CLASS (the blank included; a label that occurs twice
 *     in the target gets both shares); every row sums to 1, and y - cls is d(-log Z)/d(logits)
 *   Z == 0 (T too short, a zero posterior on every path, underflow): every occ and cls entry of the pair is +0
 * Every byte of the K n entries of each output is written.  On the device and on the host the same float32 operations in the same
 * order: ww_ctc_occupancy_dev gives the bits of ww_ctc_occupancy_rows.  Against the float64 statement on the same float32 posteriors
 * an occ entry is within (6T + 4) 2^-24 relative, a cls entry within (6T + 4 + 2U) 2^-24, plus an absolute term for what lies under
 * FLT_MIN (derived in tests/ctc_occupancy64.py).
 * WW_EINVAL before anything is written, the text naming the rule: ww_ctc_score_*'s rules, a NULL value or occ, a cls in prefix mode.
 * n = 0: WW_OK.
 * ww_ctc_occupancy_dev - ctc_occupancy_kernel alone (csrc/ctc_occupancy.hip) on any device posteriors [n][T][L], enqueued on the
 *   context's stream.
 * ww_ctc_occupancy_rows - host only, no context (its refusal's text: ww_last_error(NULL)).
 * ww_ctc_occupancy / _windows_dev / ww_ctc_slide_occupancy - ww_ctc_align / _windows_dev / ww_ctc_slide_align with this kernel in the
 *   align kernel's place behind every chunk's model launch (T = 19, L = n_out); labels / lengths are the optional decode, as there. */
int ww_ctc_occupancy_dev(ww_ctx *ctx, const float *d_steps, int64_t n, int32_t T, int32_t L, const int32_t *targets, const int32_t *target_lens,
                         int32_t K, int32_t mode, float *d_value, float *d_occ, float *d_cls);
int ww_ctc_occupancy_rows(const float *steps, int64_t n, int32_t T, int32_t L, const int32_t *targets, const int32_t *target_lens, int32_t K,
                          int32_t mode, float *value, float *occ, float *cls);
int ww_ctc_occupancy(ww_ctx *ctx, const ww_model *model, const float *windows, int32_t n, const int32_t *targets, const int32_t *target_lens,
                     int32_t K, int32_t mode, float *value, float *occ, float *cls, int32_t max_labels, int32_t *labels, int32_t *lengths);
int ww_ctc_occupancy_windows_dev(ww_ctx *ctx, const ww_model *model, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                                 const int32_t *d_win_valid, int32_t n, const int32_t *targets, const int32_t *target_lens, int32_t K,
                                 int32_t mode, float *d_value, float *d_occ, float *d_cls, int32_t max_labels, int32_t *d_labels,
                                 int32_t *d_lengths);
int ww_ctc_slide_occupancy(ww_ctx *ctx, const ww_model *model, const float *mel, int64_t rows, int32_t hop, const int32_t *targets,
                           const int32_t *target_lens, int32_t K, int32_t mode, float *value, float *occ, float *cls, int32_t max_labels,
                           int32_t *labels, int32_t *lengths, int64_t *n_windows);

/* ww_forward_windows_dev over a model set: window w is evaluated by member win_model[w], all windows in ONE launch (K checkpoints
 * over the same mel - the loop over eval_models of wwdetect/wavenet/evaluate_wavenet.py - are K x n windows that name the same rows).
 * win_model is a HOST array: read and checked before the call returns (an id outside [0, n_models): WW_EINVAL, nothing is launched),
 * sent to the device with the call's other tables.  d_enc (may be NULL) receives the encoder rows [n_windows][enc_rows][enc_width].
 * CRNN: one crnn_fused_kernel launch whatever n_windows is (no front + tail split); Wavenet: the fp32 transposed form, twelve waves
 * up to 256 windows and four above, as for one model.  Row w carries the bits of ww_forward_windows_dev with member win_model[w] on
 * the same launch size.  n_windows = 0: WW_OK, nothing written.  Extent: as ww_forward_windows_dev, for d_out and for d_enc
 * ([0, n_windows) rows each). */
int ww_set_forward_windows_dev(ww_ctx *ctx, const ww_model_set *set, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                               const int32_t *d_win_valid, const int32_t *win_model, int32_t n_windows, float *d_out, float *d_enc);

/* Several mel sequences in one device buffer (the padded clips of a test set), each slid over with the same hop:
 * sequence s has seg_nw[s] complete windows, window k of it covers rows [seg_row0[s] + k*hop, + window).
 * seg_row0 / seg_nw are HOST arrays; d_out receives the detect rows sequence by sequence.  This is the window loop of
 * utils/evaluate_models.py:66-88 over many files at once; for the CRNN the conv and the layer-1 projection of a time
 * position are computed once per sequence instead of once per window that contains it.  The host arrays are read before the
 * call returns, for every model: the caller may free or overwrite them at once.  The kernels are enqueued like every _dev entry
 * point's and the call waits for none of them unless a buffer of the context has to grow for it (its launch tables travel
 * through two page-locked buffers of the context, so a caller can stage its next batch while this one computes).
 * Extent: rows of the buffer outside every sequence - the gaps, what lies in front of the first and behind the last - never reach
 * a result (a sequence's edge positions are computed from ITS rows and zeros, whatever its neighbours hold: NaN and Inf included);
 * d_out[0 .. sum of seg_nw) is written and nothing else; a non-finite row affects the windows of its own sequence that name it,
 * and no other sequence.  A sequence gives the bits it gives in a call of its own. */
int ww_forward_segments_dev(ww_ctx *ctx, const ww_model *model, const float *d_mel, int64_t mel_rows, const int64_t *seg_row0,
                            const int32_t *seg_nw, int32_t n_seg, int32_t hop, float *d_out);

/* The same over a model set - the evaluator's form (windows SLIDING over clips, utils/evaluate_models.py:66-88) for a list of
 * checkpoints: every sequence is slid over by every member the call names.  members: a HOST array of n_members member ids, each a
 * "slot" of the call; duplicates are allowed; NULL = every member of the set in order (n_members is then not looked at, but for its
 * sign).  d_out is [slots][W][n_out], W = the sum of seg_nw, windows numbered sequence by sequence as in ww_forward_segments_dev:
 * plane k holds member members[k]'s detect rows, with the bits that member gives alone in the same form (below).
 * CRNN, hop 1..8, the sliding form enabled (WW_OPT_CRNN_SLIDE_MIN != 0) and W >= WW_OPT_CRNN_SLIDE_MIN: per group of sequences ONE
 * crnn_rows_kernel launch and ONE tail launch over a (tiles | windows) x slots grid - a slot's projected rows, tail scratch and
 * detect rows are planes of member-major buffers, the tile and first-field tables are built and uploaded once for all slots.  Groups
 * are whole sequences with slots x windows <= 32,768 (a single larger sequence is a group of its own): the workspace bound of
 * ww_forward_segments_dev.  CRNN otherwise, and every Wavenet: slots x W explicit windows naming the same rows, through the one-launch
 * form of ww_set_forward_windows_dev.
 * WW_EINVAL, with nothing enqueued and nothing written: a NULL ctx / set / d_mel / d_out (seg_row0 / seg_nw where n_seg > 0); a set
 * of another context; hop <= 0; n_seg < 0; n_members < 0; a negative seg_nw; windows that leave the mel buffer; a member id outside
 * [0, n_models) (ww_last_error names its index).  n_seg = 0, W = 0 and n_members = 0 (members != NULL) are WW_OK and write nothing.
 * The host arrays are read before the call returns; the call enqueues and waits for no kernel unless a buffer of the context has to
 * grow.
 * ww_set_slide_forward: host pointers, ONE sequence of `rows` rows, synchronous - ww_slide_forward for every slot over one upload:
 * out is [slots][n_windows][n_out], *n_windows the count PER MEMBER ((rows - window) / hop + 1, 0 if rows < window).
 * ww_set_option: WW_OPT_CRNN_SLIDE_MIN and WW_OPT_CRNN_TAIL_MFMA (ww_model_set_option's meanings and ranges) for the set's launches -
 * the two options that decide the form above - and WW_OPT_WAVE_SEQ_SEGMENT (likewise) for the cuts of ww_set_wave_sequence*; a set
 * starts from the library's defaults whatever its members' options are.  Every other key (WW_OPT_CRNN_SPLIT_AT and
 * WW_OPT_WAVENET_ROWMAJOR among them): WW_EINVAL.  The two tails give the same bits; the rows form and the explicit-window form differ as they do for one model
 * (three of a window's nineteen projected rows are summed in another order: posteriors within 2e-6).  A single model's
 * ww_forward_segments_dev takes the rows form whatever W is: WW_OPT_CRNN_SLIDE_MIN = 1 gives a set exactly those bits.
 * Extent: as ww_forward_segments_dev in every plane; the slots x W rows of d_out are written and nothing behind the last plane. */
int ww_set_forward_segments_dev(ww_ctx *ctx, const ww_model_set *set, const float *d_mel, int64_t mel_rows, const int64_t *seg_row0,
                                const int32_t *seg_nw, int32_t n_seg, int32_t hop, const int32_t *members, int32_t n_members, float *d_out);
int ww_set_slide_forward(ww_ctx *ctx, const ww_model_set *set, const float *mel, int64_t rows, int32_t hop, const int32_t *members,
                         int32_t n_members, float *out, int64_t *n_windows);
int ww_set_option(ww_model_set *set, int key, int64_t value);

/* ---- Wavenet on whole sequences (fp32) ----------------------------------------------------
 * The reference Wavenet is causal and fully convolutional: its trainer builds it with timesteps=None "for variable length"
 * (wwdetect/wavenet/train_wavenet.py:75, wavenet_model.py:165-172) and only the TFLite export freezes 182 rows.  This is that
 * reading - NOT the TFLite window form of ww_forward / ww_slide_forward, whose every window zero-pads its own left edge.
 * For a mel sequence x[0..L), any L >= 1:
 *   enc[t]     [32]     the skip sum of row t, and
 *   logits[t]  [n_out]  the head's value BEFORE the max over time, of the model evaluated on the whole sequence: causal taps
 *                       read zeros in front of row 0 and nothing else is padded;
 *   post       [n_out]  softmax(max over t of logits[t]): what model(X) returns with timesteps=None;
 *   post_frames[t]      softmax(m[t]), m[t][c] = max of logits[s][c] over max(0, t - pool_rows + 1) <= s <= t; pool_rows = 0:
 *                       from row 0.  With pool_rows = the model's window (182) this is the pool of the window form, with true
 *                       left context in place of the window's padding.
 * Row t depends on rows t - RF + 1 .. t only (RF = 1 + 2 * sum of the dilations = 181): enc[t], t >= window - 1, carries the bits
 * of row window - 1 of ww_forward_enc on the window that ends at t, and for L = window the call IS the window form.
 * Sequence s occupies rows [row_offs[s], row_offs[s + 1]) of the mel buffer (row_offs: n_seq + 1 ascending HOST entries within
 * [0, total_rows]; rows between or around the sequences are neither read nor written).  The per-row outputs are indexed by
 * mel row; post by sequence (an empty sequence's row is left as it is).  Every output may be NULL.  No limit on L: a long
 * sequence is cut into segments that run in parallel (WW_OPT_WAVE_SEQ_SEGMENT), with the same bits wherever the cuts fall.
 * WW_EINVAL for a CRNN, for a model in WW_PRECISION_BF16X3, n_seq < 0, pool_rows < 0 or descending offsets; n_seq = 0 and empty
 * sequences are no-ops.  The device form enqueues on the context's stream and does not synchronise it (but where one of the
 * context's buffers has to grow for a call larger than any before): row_offs is read before the call returns, and the caller
 * may free or overwrite it at once. */
int ww_wave_sequence_dev(ww_ctx *ctx, const ww_model *model, const float *d_mel, int64_t total_rows, const int64_t *row_offs,
                         int32_t n_seq, int32_t pool_rows, float *d_enc, float *d_logits, float *d_post_frames, float *d_post);
int ww_wave_sequence(ww_ctx *ctx, const ww_model *model, const float *mel, int64_t total_rows, const int64_t *row_offs, int32_t n_seq,
                     int32_t pool_rows, float *enc, float *logits, float *post_frames, float *post);

/* The same over a model set of Wavenets, in ONE call over ONE mel buffer: the checkpoint loop of
 * wwdetect/wavenet/evaluate_wavenet.py: eval_models over whole recordings (_all), and a service whose recordings each belong to a
 * tenant's member (by sequence).  Sequences, row_offs, pool_rows and the outputs' meaning are ww_wave_sequence's.
 *   ww_set_wave_sequence[_dev]: sequence s is evaluated by member seq_model[s] (a HOST array of n_seq ids; NULL = every sequence by
 *     member 0); the outputs are laid out as ww_wave_sequence's - one plane.
 *   ww_set_wave_sequence_all[_dev]: every sequence by every slot.  members / n_members as in ww_set_forward_segments_dev: a HOST array
 *     of member ids, each a slot of the call, duplicates allowed, NULL = every member of the set in order (n_members is then looked at
 *     for its sign only).  Plane k is member members[k]: enc [slots][total_rows][32], logits and post_frames
 *     [slots][total_rows][n_out], post [slots][n_seq][n_out].
 * Every output of sequence s in plane k carries the bits ww_wave_sequence gives for that sequence with that member alone, wherever the
 * cuts fall (ww_set_option: WW_OPT_WAVE_SEQ_SEGMENT) and whatever the neighbouring sequences, the other slots and the size of the call
 * are.  Rows of the buffers outside every sequence are neither read nor written, in every plane; an empty sequence's post rows are
 * left as they are.  Every output may be NULL.
 * The model kernel runs ONCE for all planes (a segments x slots grid, 1,024 slots per launch; the segment table is the single
 * model's, the members travel beside it) and so does each pooling kernel: the launch count does not grow with the slots.
 * WW_EINVAL, with nothing enqueued and nothing written: a NULL ctx or set; a set of another context; a set of CRNNs (a CRNN's
 * bidirectional GRUs have no causal reading); n_seq < 0, pool_rows < 0, n_members < 0; offsets that descend or leave the buffer; a
 * member id outside [0, n_models) (ww_last_error names its index); a NULL mel buffer where there are rows to compute.  WW_OK with
 * nothing written: n_seq = 0, all sequences empty, n_members = 0 with members != NULL, every output NULL.
 * The _dev forms enqueue on the context's stream and wait for nothing unless a buffer of the context has to grow; their host arrays
 * are read before the call returns.  The host forms upload the mel once, whatever the number of slots, and are synchronous. */
int ww_set_wave_sequence_dev(ww_ctx *ctx, const ww_model_set *set, const float *d_mel, int64_t total_rows, const int64_t *row_offs,
                             int32_t n_seq, const int32_t *seq_model, int32_t pool_rows, float *d_enc, float *d_logits,
                             float *d_post_frames, float *d_post);
int ww_set_wave_sequence(ww_ctx *ctx, const ww_model_set *set, const float *mel, int64_t total_rows, const int64_t *row_offs,
                         int32_t n_seq, const int32_t *seq_model, int32_t pool_rows, float *enc, float *logits, float *post_frames,
                         float *post);
int ww_set_wave_sequence_all_dev(ww_ctx *ctx, const ww_model_set *set, const float *d_mel, int64_t total_rows, const int64_t *row_offs,
                                 int32_t n_seq, int32_t pool_rows, const int32_t *members, int32_t n_members, float *d_enc,
                                 float *d_logits, float *d_post_frames, float *d_post);
int ww_set_wave_sequence_all(ww_ctx *ctx, const ww_model_set *set, const float *mel, int64_t total_rows, const int64_t *row_offs,
                             int32_t n_seq, int32_t pool_rows, const int32_t *members, int32_t n_members, float *enc, float *logits,
                             float *post_frames, float *post);

/* Whole hot path for a batch of equal-length clips resident in HBM (BASELINE configs 2/3):
 * PCM [n_clips][samples_per_clip] -> log-mel -> one zero-padded window per clip ->
 * encode + detect -> d_out [n_clips][n_out].  d_mel_scratch may be NULL (ctx workspace).
 * A clip has (samples_per_clip - 512) / hop + 1 frames.  A clip of fewer than 512 samples has none and yields the model's row
 * for the all-zero window; a clip of more than `window` frames is judged by its first `window` frames, the rest is not read by
 * the model.  The result for a clip does not depend on the batch it is in (tests/test_gpu_clips64.py pins all of this).
 * d_pcm is 16-byte aligned; WW_EINVAL for more than 65535 clips, a negative size, a hop outside 1..512, a pcm_divisor that is
 * not positive or a NULL buffer; n_clips = 0 is a no-op.
 * Extent: samples in front of d_pcm and behind its n_clips x samples_per_clip never reach a result; d_out[0 .. n_clips) is written
 * and nothing else. */
int ww_clips_forward_dev(ww_ctx *ctx, const ww_model *model, const int16_t *d_pcm, int32_t n_clips,
                         int32_t samples_per_clip, const ww_frontend_params *fp, float *d_out);

/* ---- streaming (spokestack/pipeline.py + WakewordTrigger, BASELINE config 5) -------------
 * S independent 16 kHz streams advanced in lock step, 20 ms per tick.  Device-resident
 * state per stream: sample ring (512), mel window ring (window x 40), pre-emphasis carry,
 * running posterior max (tflite.py:96-108).  Per tick and stream: 0..2 new mel frames; for
 * each new frame while is_speech[s] != 0 one encode+detect (tflite.py:163-168,187-215).
 * post[s][k] (k < n_post[s] <= 2) are the posteriors produced by this tick, in order.
 * is_speech[s] is a bit set: bit 0 = the VAD says speech (context.is_speech); bit 1 = the stream is already
 * active (context.is_active): the reference does not sample an active stream at all (tflite.py:139-140), so its
 * rings stand still and it yields no posterior until the flag is cleared.  frames = [n_streams][320] int16
 * (20 ms at 16 kHz). */
/* flags: WW_STREAM_FULL_RECOMPUTE = every streaming CRNN window recomputed from its mel rows by the batch kernels instead of
 * the incremental crnn_stream_kernel (3 new time positions per window); results agree to 2e-6.  0 = default. */
#define WW_STREAM_FULL_RECOMPUTE 1u
/* Round 5: a tick of the incremental CRNN bank is ONE kernel launch - the front end of a stream's new frames runs inside the
 * workgroups of that stream's new windows - and ww_stream_step waits for a tick's posteriors by polling {value, tick number}
 * pairs the kernels store into page-locked memory instead of the runtime's completion signal (every bank whose context owns
 * its stream; on a borrowed stream the call still returns only when the stream has drained).  Same bits either way.
 * WW_STREAM_TWO_LAUNCH keeps the front-end kernel + model kernel form, WW_STREAM_SYNC_WAIT the hipStreamSynchronize wait:
 * the forms the tests compare against. */
#define WW_STREAM_TWO_LAUNCH 2u
#define WW_STREAM_SYNC_WAIT 4u
/* WW_STREAM_CAUSAL (fp32 Wavenet only, else WW_EINVAL; not together with WW_STREAM_FULL_RECOMPUTE): the bank advances the
 * sequence form of ww_wave_sequence one mel row at a time from cached activations instead of recomputing a window per row.  Per
 * stream it keeps the blocks' last 16 rows of BatchNorm output (24 KB), a ring of the last `window` logit rows and a row count.
 * EVERY sampled mel row advances that state, whatever bit 0 of is_speech says (the history must not have holes); posteriors are
 * emitted under the usual rule - for rows that arrive while bit 0 is set - and are post_frames[t][posterior column] of
 * ww_wave_sequence with pool_rows = window over the stream's rows since its last reset, bit for bit.  Bit 1 freezes the stream
 * as always; ww_stream_reset zeroes the causal state: the next row is row 0 of a new sequence.  A tick is the front-end kernel
 * and one model kernel, with either wait.  Without the flag nothing changes. */
#define WW_STREAM_CAUSAL 8u
int ww_stream_create(ww_ctx *ctx, const ww_model *model, int32_t n_streams, const ww_frontend_params *fp, uint32_t flags,
                     ww_streams **out);
/* A bank whose streams each have a model of a set (one wake word per tenant: one bank, one front end, one tick).  stream_model[s] is
 * the member that serves stream s - a HOST array, checked here (an id outside [0, n_models): WW_EINVAL), NULL = all 0 - and the bank
 * keeps it as a device table.  Every ww_stream_* call and ww_pipeline_bank_step work on such a bank unchanged; stream s yields the
 * bits it yields in a bank of member stream_model[s] alone.  Forms: the incremental CRNN bank (one launch, WW_STREAM_TWO_LAUNCH, both
 * waits), the Wavenet window bank (one launch and WW_STREAM_TWO_LAUNCH), WW_STREAM_CAUSAL by tick and by ww_stream_feed.
 * WW_STREAM_FULL_RECOMPUTE on a set: WW_EINVAL.  The set must outlive the bank.
 * ww_stream_set_model moves the listed streams (ids NULL -> all) to member `model` AND resets them as ww_stream_reset does - a
 * stream's cached activations belong to the model that made them -, in stream order with the ticks.  WW_EINVAL: a bank that was not
 * created from a set, an id or a model out of range.  A failure after the bank's table has changed marks the bank broken (WW_ESTATE
 * from then on), as a failed tick does. */
int ww_stream_create_set(ww_ctx *ctx, const ww_model_set *set, int32_t n_streams, const int32_t *stream_model,
                         const ww_frontend_params *fp, uint32_t flags, ww_streams **out);
int ww_stream_set_model(ww_streams *st, const int32_t *ids, int32_t n, int32_t model);
/* A bank that runs EVERY listed member of a set on EVERY stream (a device that listens for several wake words at once: one audio
 * stream, K posteriors per 20 ms).  `members` is a HOST array of K = n_members member slots, 1 <= K <= 64, each checked as
 * ww_stream_create_set's ids are; a member may be named more than once; NULL = every member of the set in order (n_members is then
 * ignored).  Flags: 0, WW_STREAM_TWO_LAUNCH, WW_STREAM_SYNC_WAIT, and WW_STREAM_CAUSAL for a Wavenet set; WW_STREAM_FULL_RECOMPUTE
 * and n_streams * K > 65535 are WW_EINVAL.  One front end per stream serves all K slots: a tick takes the frames of S streams once,
 * and the bank keeps one sample ring and one mel history per stream and one model state per stream and slot.
 * ww_stream_step_all is the bank's tick: frames, is_speech and n_post [S] exactly as ww_stream_step's; post is [S][K][2],
 * post[s][j][k] = the posterior of member slot j for the tick's new row k (0 for k >= n_post[s]) - the bits a bank of that member
 * alone yields on the same frames, flags and resets.  Forms: the incremental CRNN in one launch (default) and two, both waits; the
 * Wavenet window bank (always two launches); WW_STREAM_CAUSAL by tick.
 * ww_stream_members reads the list back: members (K entries; may be NULL) and *n_members = K; an ordinary bank: *n_members = 0.
 * On such a bank ww_stream_reset (a stream's front end and all K model states), ww_stream_window, ww_stream_attach_resampler,
 * ww_stream_attach_rates, ww_stream_set_rate, ww_stream_frame_samples, ww_stream_frame_layout, ww_stream_timeline and
 * ww_stream_destroy work unchanged; ww_stream_feed_all / ww_stream_feed_rows_all feed a WW_STREAM_CAUSAL bank of this kind in
 * packets, and ww_stream_step_trigger_all is its wake-word stage (both further down).  WW_EINVAL with the reason in ww_last_error,
 * before any state moves: ww_stream_step, ww_stream_step_trigger, ww_pipeline_bank_step, ww_stream_set_model, ww_stream_feed and
 * ww_stream_feed_rows on an every-member bank; ww_stream_step_all, ww_stream_feed_all, ww_stream_feed_rows_all and
 * ww_stream_step_trigger_all on any other bank. */
int ww_stream_create_set_all(ww_ctx *ctx, const ww_model_set *set, int32_t n_streams, const int32_t *members, int32_t n_members,
                             const ww_frontend_params *fp, uint32_t flags, ww_streams **out);
int ww_stream_step_all(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, float *post, int32_t *n_post);
int ww_stream_members(const ww_streams *st, int32_t *members, int32_t *n_members);
int ww_stream_destroy(ww_streams *st);
int ww_stream_step(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, float *post, int32_t *n_post);
/* WakewordTrigger.reset (tflite.py:241-246) for the listed streams (ids NULL -> all). */
int ww_stream_reset(ww_streams *st, const int32_t *ids, int32_t n);
/* Read-out for tests and tools: stream `stream`'s newest mel window - the T x n_mel block the model reads, the T rows that end at
 * the last row written (all-zero rows in front of a stream's first rows and after a reset) - copied to host memory `out`
 * (T * n_mel floats, row-major) after the context's stream has been synchronised.  Touches no state of the bank.  WW_EINVAL for
 * a stream id out of range. */
int ww_stream_window(ww_streams *st, int32_t stream, float *out);
/* ww_stream_feed - a WW_STREAM_CAUSAL bank advanced by ANY subset of its streams and ANY number of samples for each (packets of
 * 10 .. 100 ms, a backlog of minutes): stream ids[i] receives samples [sample_offs[i], sample_offs[i + 1]) of pcm, any count >= 0.
 * Framing is the tick's rule for k samples: a stream holds fill <= 511 pending samples; tot = fill + k,
 * rows = tot >= 512 ? (tot - 512) / 160 + 1 : 0, fill' = tot - 160 rows.  Every new mel row advances the causal state and yields
 * one posterior - post_frames[t][posterior column] of ww_wave_sequence with pool_rows = window over the stream's rows since its
 * last reset, the tick's definition.  However a stream's samples are cut into packets, calls and ww_stream_step ticks, the mel
 * rows, the posteriors and the state left behind are the same bits; ww_stream_step / _reset / _window work on a fed bank as before.
 *   row_offs [n + 1]            written: stream ids[i]'s new rows are [row_offs[i], row_offs[i + 1]) of post and mel
 *   post [row_offs[n]]          one posterior (the posterior column, as ww_stream_step's) per new mel row, stream by stream
 *   mel  [row_offs[n]][n_mel]   the new mel rows themselves; may be NULL
 *   cap_rows                    rows `post` (and `mel`) have room for
 * There is no is_speech: a stream that must stand still is not named.  WW_EINVAL - before any state changes - for a bank without
 * WW_STREAM_CAUSAL, NULL arguments, n < 0, an id out of range or named twice, descending sample_offs, cap_rows smaller than the
 * rows of the call; WW_ESTATE for a bank marked broken; WW_ENOMEM when the call's scratch (samples, rows, logits; it grows on
 * demand) cannot be had.  n = 0, empty packets and packets that leave a stream below 512 samples are no-ops for the model (the
 * samples are kept).  A failure after the host's mirrors advanced marks the bank broken, as a tick's does.  The call ends in
 * hipStreamSynchronize on the context's stream (a ragged result has no tag slots); it works on a borrowed stream.
 * ww_stream_feed_rows writes the row_offs the same call would produce and touches no state: what to size post / mel by. */
int ww_stream_feed_rows(ww_streams *st, const int32_t *ids, int32_t n, const int64_t *sample_offs, int64_t *row_offs);
int ww_stream_feed(ww_streams *st, const int32_t *ids, int32_t n, const int16_t *pcm, const int64_t *sample_offs, int64_t cap_rows,
                   int64_t *row_offs, float *post, float *mel);
/* ww_stream_feed_all - ww_stream_feed on a bank created by ww_stream_create_set_all with WW_STREAM_CAUSAL (K member slots per
 * stream): the same arguments and the same semantics, with
 *   row_offs [n + 1]            counts MEL rows (not rows x K): stream ids[i]'s new rows are [row_offs[i], row_offs[i + 1])
 *   post [row_offs[n]][K]       post[r][j] = the posterior of member slot j for new mel row r
 *   mel  [row_offs[n]][n_mel]   written once per physical stream; may be NULL
 * Slot j of stream s yields, bit for bit, what ww_stream_feed yields on an ordinary causal bank of member members[j] alone given the
 * same packets, resets and ticks: a stream's samples may be cut into ww_stream_feed_all packets, calls and ww_stream_step_all ticks
 * in any way.  The samples are uploaded and the front end runs once per stream whatever K is; each model segment runs once per slot.
 * WW_EINVAL - before any state changes - for everything ww_stream_feed refuses, a bank that was not created by
 * ww_stream_create_set_all, an every-member bank without WW_STREAM_CAUSAL, and a call of more than 2^30 posteriors (rows x K);
 * WW_ESTATE, WW_ENOMEM and the broken-bank rule as ww_stream_feed's.  On any refusal row_offs, post and mel are left as they were.
 * ww_stream_feed_rows_all writes the row_offs the same call would produce and touches no state. */
int ww_stream_feed_rows_all(ww_streams *st, const int32_t *ids, int32_t n, const int64_t *sample_offs, int64_t *row_offs);
int ww_stream_feed_all(ww_streams *st, const int32_t *ids, int32_t n, const int16_t *pcm, const int64_t *sample_offs, int64_t cap_rows,
                       int64_t *row_offs, float *post, float *mel);
/* ---- a stream bank at another input rate than 16 kHz ----------------------------------------------------------------------------
 * ww_stream_attach_resampler makes `st` a bank at r's input rate: ww_stream_step, ww_stream_step_trigger and ww_pipeline_bank_step
 * then read `frames` as [S][F] int16, F = rate_in / 50 (ww_stream_frame_samples: F, or 320 for a plain bank), and ww_stream_feed /
 * ww_stream_feed_rows take packets at rate_in.  One kernel in front of a tick's own resamples the S frames into the [S][320] block
 * the tick kernels read; no other kernel of the bank changes, so every form a bank has (ww_stream_create and ww_stream_create_set;
 * incremental CRNN in one and two launches, both waits, WW_STREAM_FULL_RECOMPUTE, the Wavenet window bank in one and two launches,
 * WW_STREAM_CAUSAL) works at rate_in.
 * Definition.  r has (up, down, half) (ww_resampler_info).  Let x be the samples a stream has received since its last reset,
 * LEAVING OUT the frames of ticks in which bit 1 of is_speech froze it (a frozen stream's frame is dropped whole, as its 16 kHz
 * frame is, and its resampling state stands still), y = ww_resample's int16 output for x (out_format WW_SAMPLE_I16) continued as
 * if x went on, and D = ceil(half / down).  The stream's 16 kHz signal is
 *     z[n] = 0 for n < D,   z[n] = y[n - D] for n >= D
 * and after N input samples the bank has consumed exactly floor(N * up / down) samples of z - 320 per tick, each determined by
 * the N samples because half < down * (D + 1); the delay (D = 34 samples, 2.1 ms, for the default filter at every standard rate
 * >= 16 kHz, 68 at 8 kHz) is what lets a tick deliver 320 samples from the first tick on.  A bank at rate_in yields, for every
 * stream and every call, THE BITS OF THE SAME BANK AT 16 kHz GIVEN z.  A fed stream with N inputs and k new ones advances by
 * floor((N + k) * up / down) - floor(N * up / down) samples of z, to which the tick's framing rule applies; however a stream's
 * samples are cut into packets, calls and ticks, the bits are the same.  ww_stream_reset and ww_stream_set_model also clear the
 * listed streams' resampling state (the next sample is x[0], z starts with D zeros again).  A stream keeps
 * max(ceil((D * down + half) / up) + 1, ceil(((D + 1) * down + half) / up)) input samples between calls.
 * Allowed only on a bank that has neither ticked nor been fed since its creation (else WW_ESTATE).  WW_EINVAL, ww_last_error
 * naming the reason: r of another context, rate_out != 16000, rate_in == 16000 (a plain bank), rate_in % 50 != 0 (a fractional
 * 20 ms frame - 11025 Hz has 220.5 samples -: not offered in the tick; resample such a stream in front of the bank), a second
 * attach, a geometry whose history + frame exceed what a tick stages (12288 samples).  The resampler must outlive the bank. */
int ww_stream_attach_resampler(ww_streams *st, const ww_resampler *r);
int ww_stream_frame_samples(const ww_streams *st, int32_t *out);
/* ---- a stream bank whose streams each run at their own sample rate ---------------------------------------------------------------
 * ww_stream_attach_rates makes `st` a bank whose stream s runs at the input rate of rate class stream_rate[s]: 8 kHz telephony legs,
 * 16 kHz app audio and 44.1 / 48 kHz capture streams in ONE bank and ONE tick.  rs[k] is class k (up to WW_STREAM_MAX_RATES);
 * rs[k] == NULL is the 16 kHz class, a pass-through with no delay and no history.  stream_rate [n_streams] is a HOST array, read and
 * checked before the call returns; NULL = every stream in class 0.  One kernel launch in front of a tick's own serves all classes;
 * no other kernel of the bank changes, so every form a bank has works (as ww_stream_attach_resampler lists them).
 * Contract.  Stream s yields, for every call (tick, trigger step, pipeline step, feed, window read-out), THE BITS STREAM s YIELDS
 * IN A BANK THAT RUNS AT ITS RATE ALONE: for the 16 kHz class the plain bank, for any other class the bank
 * ww_stream_attach_resampler(rs[k]) makes - z is the resampled signal behind D zeros, as defined above.
 * Frames.  `frames` of ww_stream_step, ww_stream_step_trigger and ww_pipeline_bank_step is ONE contiguous ragged int16 block:
 * stream s's rate / 50 samples start at sample frame_offs[s], no padding between streams.  ww_stream_frame_layout writes
 * frame_samples [n_streams] and frame_offs [n_streams + 1] (frame_offs[n_streams] = the block's samples); it works on every bank (a
 * plain or single-rate bank: the uniform layout).  ww_stream_frame_samples on a bank with per-stream rates is WW_EINVAL.
 * ww_stream_feed / ww_stream_feed_rows on a WW_STREAM_CAUSAL bank: stream ids[i]'s packet is at that stream's rate, the rows follow
 * from floor((N + k) * up / down) - floor(N * up / down) with the stream's own class (the 16 kHz class: the plain rule); however a
 * stream's samples are cut into packets, calls and ticks, the bits are the same.  A feed's launches and copies are per class present
 * in the call, whatever the number of streams.
 * ww_stream_set_rate moves the listed streams (ids NULL -> all) to class rate_class AND resets them as ww_stream_reset does - the
 * resampling count included: the next sample is x[0] of a new signal -, in stream order with the ticks, as ww_stream_set_model.
 * The layout changes with it: read ww_stream_frame_layout again.  WW_EINVAL: a bank without rates, an id or a class out of range.
 * A failure after the bank's table has changed marks the bank broken.  ww_stream_reset and ww_stream_set_model clear the listed
 * streams' resampling state, as on a single-rate bank.
 * ww_stream_attach_rates is allowed only on a bank that has neither ticked nor been fed (else WW_ESTATE); the resamplers must outlive
 * the bank.  WW_EINVAL, ww_last_error naming the class and the reason: n_rates outside 1..WW_STREAM_MAX_RATES, a class that
 * ww_stream_attach_resampler would refuse (rate_out != 16000, a resampler from 16000 - that class is NULL -, a fractional 20 ms
 * frame, a geometry too long to stage), two classes of the same input rate, more than one NULL class, stream_rate[s] outside
 * [0, n_rates) (its index named), a bank that already has a resampler or rates, a resampler of another context. */
#define WW_STREAM_MAX_RATES 8
int ww_stream_attach_rates(ww_streams *st, const ww_resampler *const *rs, int32_t n_rates, const int32_t *stream_rate);
int ww_stream_frame_layout(const ww_streams *st, int32_t *frame_samples, int64_t *frame_offs);
int ww_stream_set_rate(ww_streams *st, const int32_t *ids, int32_t n, int32_t rate_class);
/* ---- stream banks that read G.711 ------------------------------------------------------------------------------------------------
 * A telephony leg arrives as G.711, one byte per sample (WW_SAMPLE_MULAW, WW_SAMPLE_ALAW above).  A bank takes it as it is: the one
 * kernel in front of a tick, and a feed's splice and pass-through copy, decode the bytes where they unpack them.  Contract, as
 * everywhere: A G.711 STREAM YIELDS THE BITS THE SAME CALL YIELDS ON ITS DECODED int16 SAMPLES, no tolerance.  Nothing behind the rate
 * kernel knows the format, so every bank form, model-set banks, every-member banks, ww_stream_set_rate, ww_stream_reset and
 * ww_stream_set_model work on such a bank.
 * ww_stream_attach_rates_fmt is ww_stream_attach_rates where class k reads its frames and packets as formats[k]: WW_SAMPLE_I16,
 * WW_SAMPLE_MULAW or WW_SAMPLE_ALAW (WW_SAMPLE_F32 or anything else: WW_EINVAL).  A class is a (rate, format) pair: the same rate may
 * come in two formats, two classes of the same pair are WW_EINVAL.  rs[k] == NULL with a G.711 format is 16 kHz G.711: it decodes
 * only, no delay and no history (and may stand beside the int16 NULL class).  formats == NULL: all WW_SAMPLE_I16 - the call then IS
 * ww_stream_attach_rates, which keeps every refusal it has.
 * ww_stream_attach_resampler_fmt is the uniform bank of ww_stream_attach_resampler (no per-stream descriptor) whose frames are
 * [S][F] of in_format and whose packets are of in_format.
 * Frames.  On a bank that has a G.711 class, `frames` of ww_stream_step, _step_all, _step_trigger, _step_trigger_all and
 * ww_pipeline_bank_step is read as ONE BYTE block: a G.711 frame (rate / 50 bytes) starts at the next byte, an int16 frame (rate / 25
 * bytes) at the next even byte, with one pad byte in front of it where needed.  ww_stream_frame_layout_bytes writes frame_bytes
 * [n_streams], byte_offs [n_streams + 1] (byte_offs[n_streams] = the end of the last frame: the block's bytes) and formats
 * [n_streams]; it works on every bank (a plain bank: 640-byte WW_SAMPLE_I16 frames; any bank without G.711: twice
 * ww_stream_frame_layout's figures).  The layout changes with ww_stream_set_rate.  On a bank with a G.711 class the calls that count
 * int16 samples - ww_stream_frame_layout, ww_stream_frame_samples, ww_stream_feed, ww_stream_feed_all - are WW_EINVAL;
 * ww_stream_feed_rows / _rows_all count samples, whatever their format, and stay as they are.
 * ww_stream_feed_bytes / ww_stream_feed_bytes_all are ww_stream_feed / ww_stream_feed_all with packets given in bytes: packet i is
 * bytes [byte_offs[i], byte_offs[i + 1]) of data, in its stream's format.  An int16 packet with an odd offset or an odd length is
 * WW_EINVAL.  On a bank without G.711 classes they are ww_stream_feed / _all with sample_offs = byte_offs / 2.  Everything those calls
 * promise carries over: the same bits however the samples are cut into packets, calls and ticks, every refusal before any state
 * moves (row_offs, post and mel untouched), the broken-bank rule.  A call's packets go up once. */
int ww_stream_attach_rates_fmt(ww_streams *st, const ww_resampler *const *rs, const int32_t *formats, int32_t n_rates, const int32_t *stream_rate);
int ww_stream_attach_resampler_fmt(ww_streams *st, const ww_resampler *r, int32_t in_format);
int ww_stream_frame_layout_bytes(const ww_streams *st, int32_t *frame_bytes, int64_t *byte_offs, int32_t *formats);
int ww_stream_feed_bytes(ww_streams *st, const int32_t *ids, int32_t n, const void *data, const int64_t *byte_offs, int64_t cap_rows,
                         int64_t *row_offs, float *post, float *mel);
int ww_stream_feed_bytes_all(ww_streams *st, const int32_t *ids, int32_t n, const void *data, const int64_t *byte_offs, int64_t cap_rows,
                             int64_t *row_offs, float *post, float *mel);
/* ---- the pipeline's host stages for S streams in lock step (BASELINE config 5 at the plugin surface) --------------------------
 * The reference drives three stage objects per stream and 20 ms frame (spokestack/pipeline.py:25-28, stage list of demo.py:29-36),
 * each a few comparisons on the shared SpeechContext.  For S streams each stage is ONE pass over plain arrays the caller owns
 * (uint8 is_speech[S] / is_active[S] are the S SpeechContexts' flags, wwhip/context.py: ContextBank); a stage returns the ids whose
 * flag it changed, so that activate / deactivate events (spokestack/context.py:71-85) are raised for those streams only.  No GPU
 * call in the first three; ctx-less, errors are WW_EINVAL.
 *
 * ww_vad_bank_step - VoiceActivityDetector.__call__ after the classifier (spokestack/vad/webrtc.py:59-77): raw[s] = the frame
 * classifier's decision; run_value / run_length = the detector's run state; is_speech is read and updated in place;
 * rise_frames / fall_frames = vad_rise_delay // frame_width, vad_fall_delay // frame_width.  n_changed (may be NULL) = streams
 * whose is_speech moved. */
int ww_vad_bank_step(int32_t n_streams, const uint8_t *raw, int32_t rise_frames, int32_t fall_frames, uint8_t *run_value,
                     int64_t *run_length, uint8_t *is_speech, int32_t *n_changed);
/* ww_trigger_bank_step - WakewordTrigger.__call__ around the models (spokestack/wakeword/tflite.py:134-146,232-239) over the
 * posteriors post[S][2] / n_post[S] a tick delivered: running maximum, `posterior > threshold` (float32 against a Python
 * float: compared in double), is_active[s] set for the streams that fire and were not active (their ids -> fired_ids), VAD
 * falling edges against was_speech (updated) -> fall_ids, whose posterior_max is cleared; the caller resets those streams
 * (ww_stream_reset).  fired_ids / fall_ids hold up to S entries. */
int ww_trigger_bank_step(int32_t n_streams, const uint8_t *is_speech, uint8_t *is_active, const float *post, const int32_t *n_post,
                         double threshold, uint8_t *was_speech, float *posterior_max, int32_t *fired_ids, int32_t *n_fired,
                         int32_t *fall_ids, int32_t *n_fall);
/* ww_timeout_bank_step - ActivationTimeout.__call__ (spokestack/activation_timeout.py:25-38): min_frames / max_frames are
 * min_active / frame_width and max_active / frame_width as the reference keeps them (floats); is_active[s] cleared and
 * active_frames[s] zeroed for the streams that time out (-> deact_ids). */
int ww_timeout_bank_step(int32_t n_streams, const uint8_t *is_speech, uint8_t *is_active, uint8_t *was_speech, int32_t *active_frames,
                         double min_frames, double max_frames, int32_t *deact_ids, int32_t *n_deact);
/* ww_stream_step_trigger - the wake-word stage of S streams as ONE call: ww_stream_step with bit 0 = is_speech[s], bit 1 =
 * is_active[s] as they stand before the tick, ww_trigger_bank_step over its posteriors, ww_stream_reset of the streams whose
 * VAD bit fell (tflite.py:143-146). */
int ww_stream_step_trigger(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, uint8_t *is_active, double threshold,
                           uint8_t *was_speech, float *posterior_max, float *post, int32_t *n_post, int32_t *fired_ids,
                           int32_t *n_fired, int32_t *fall_ids, int32_t *n_fall);
/* ww_trigger_bank_step_all - the trigger stage that says WHICH wake word fired: ww_trigger_bank_step's rule per stream with
 * K = n_members member slots (1..64), over post[S][K][2] / n_post[S] as ww_stream_step_all delivers them.  thresholds [K]: slot j
 * EXCEEDS on a row when (double)posterior > thresholds[j].  posterior_max [S][K] is the running maximum per slot, cleared for all K
 * slots on the VAD falling edge.  A stream that is not active FIRES when any slot exceeds on any of the tick's rows: is_active[s] is
 * set - once: a context has one flag - and entry i of three parallel lists of up to S entries is written:
 *   fired_ids[i]   the stream
 *   fired_mask[i]  bit j set when slot j exceeded on any row of the tick
 *   fired_slot[i]  the winner: on the earliest row on which any slot exceeded, the exceeding slot with the greatest posterior; on
 *                  equal posteriors the lowest slot
 * A stream that is already active does not fire again (it is not listed; its maxima still move).  fall_ids as
 * ww_trigger_bank_step's.  With K = 1 and thresholds[0] = t the call IS ww_trigger_bank_step(..., t, ...), bit for bit, with
 * fired_slot all 0 and fired_mask all 1.  WW_EINVAL: NULL arguments, n_post outside 0..2, n_members outside 1..64.
 * ww_stream_step_trigger_all - the wake-word stage of an every-member bank as ONE call: ww_stream_step_all with bit 0 =
 * is_speech[s], bit 1 = is_active[s] as they stand before the tick, the rule above over its posteriors, ww_stream_reset of the
 * streams whose VAD bit fell.  WW_EINVAL with the reason in ww_last_error on a bank that was not created by
 * ww_stream_create_set_all. */
int ww_trigger_bank_step_all(int32_t n_streams, int32_t n_members, const uint8_t *is_speech, uint8_t *is_active, const float *post,
                             const int32_t *n_post, const double *thresholds, uint8_t *was_speech, float *posterior_max,
                             int32_t *fired_ids, int32_t *fired_slot, uint64_t *fired_mask, int32_t *n_fired, int32_t *fall_ids,
                             int32_t *n_fall);
int ww_stream_step_trigger_all(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, uint8_t *is_active,
                               const double *thresholds, uint8_t *was_speech, float *posterior_max, float *post, int32_t *n_post,
                               int32_t *fired_ids, int32_t *fired_slot, uint64_t *fired_mask, int32_t *n_fired, int32_t *fall_ids,
                               int32_t *n_fall);
/* ww_pipeline_bank_step - ONE tick of the whole stage list of demo.py:29-36 for S streams (spokestack/pipeline.py:25-28: for stage in
 * stages: stage(context, frame)) as one call: ww_vad_bank_step, ww_stream_step_trigger, ww_timeout_bank_step in this order on the
 * arrays the state block points to (the caller owns them all; the block itself may be reused from tick to tick).  Equivalent to
 * the three calls, stage by stage; what it saves is two trips through the host language's call layer per tick (wwhip/pipeline.py:
 * SpeechPipelineBank takes it when its stages are exactly VadBank, WakewordBank, ActivationTimeoutBank).  On return n_vad_changed,
 * n_fired / fired_ids, n_fall / fall_ids, n_deact / deact_ids say which streams changed. */
typedef struct ww_pipeline_state {
  uint8_t *is_speech, *is_active;          /* the S contexts' flags (updated in place) */
  const uint8_t *raw;                      /* VAD: the classifier's decisions of this tick */
  uint8_t *run_value;                      /*      run state */
  int64_t *run_length;
  uint8_t *wake_was_speech;                /* wake word: VAD edge detector, */
  float *posterior_max, *post;             /*            running maxima [S], this tick's posteriors [S][2] */
  int32_t *n_post;                         /*            and their counts [S] */
  uint8_t *timeout_was_speech;             /* timeout: VAD edge detector, */
  int32_t *active_frames;                  /*          frames since activation [S] */
  int32_t *fired_ids, *fall_ids, *deact_ids; /* out: ids (up to S each) */
  double threshold, min_frames, max_frames;
  int32_t rise_frames, fall_frames;
  int32_t n_vad_changed, n_fired, n_fall, n_deact; /* out */
} ww_pipeline_state;
int ww_pipeline_bank_step(ww_streams *st, const int16_t *frames, ww_pipeline_state *ps);
/* ---- CTC stream banks: a CTC-trained CRNN (WW_HEAD_CTC) behind the streaming tick ---------------------------------------------
 * ww_stream_create, ww_stream_create_set[_all] and ww_model_set_create refuse a CTC model; this is its own way in.
 * ww_stream_create_ctc - S streams in lock step on ONE fp32 CTC-trained CRNN.  flags: 0, WW_STREAM_TWO_LAUNCH, WW_STREAM_SYNC_WAIT,
 * WW_STREAM_FULL_RECOMPUTE (as ww_stream_create's) and WW_STREAM_CTC_STEPS; WW_STREAM_CAUSAL, an unknown flag, and a model that is
 * not an fp32 WW_HEAD_CTC CRNN are WW_EINVAL.  The default form is the incremental kernel in one launch per tick (3 new time
 * positions per window, the rest from the per-stream cache) with layer 2's nineteen steps, the per-row softmax head and the greedy
 * decode inside the workgroup; a window's decode travels to the host as one 32-bit word (bits 27..31 the whole decoded length 0..19,
 * bits 3i..3i+2 label i for i < WW_STREAM_CTC_MAX_LABELS; a label is < L - 1 <= 7).  With WW_STREAM_FULL_RECOMPUTE a tick's windows
 * go through the offline path's kernels (ww_ctc_forward's: front + CTC tail) over the ring's descriptors, and carry ITS bits; the
 * incremental forms agree with one another bit for bit and with the offline path within the bound the incremental CRNN bank has
 * against ww_forward.  WW_STREAM_CTC_STEPS: the bank also returns every window's [19][L] posteriors; such a bank always waits with
 * hipStreamSynchronize (no order is built between the posteriors' stores and a polled tag).
 * ww_stream_step_ctc - the tick.  frames, is_speech (bit 0 = speech, bit 1 = active) and n_post [S] exactly as ww_stream_step's; for
 * each of the 0, 1 or 2 new windows k of stream s: labels [S][2][max_labels] the first decoded labels padded with -1, lengths [S][2]
 * the WHOLE decoded length (it may exceed max_labels), steps [S][2][19][L] the posteriors (may be NULL; non-NULL on a bank without
 * WW_STREAM_CTC_STEPS is WW_EINVAL).  1 <= max_labels <= WW_STREAM_CTC_MAX_LABELS.  Entries at or past n_post[s] are left as they were.
 * ww_ctc_trigger_bank_step / ww_stream_step_ctc_trigger - the wake-word stage: ww_trigger_bank_step and ww_stream_step_trigger with
 * another firing rule - the same VAD-edge bookkeeping against was_speech, the same fired and fall lists, the same reset of the
 * streams whose speech bit fell.  A stream that is not active fires on the first window of the tick whose decode STARTS WITH
 * target[0 .. n_target): its whole length reaches n_target and its first n_target labels equal it (wwdetect/CRNN/evaluate.py:100-150
 * with [HEY][SNIPS]); 1 <= n_target <= max_labels.
 * On a CTC bank ww_stream_reset, _window, _attach_resampler[_fmt], _attach_rates[_fmt], _set_rate, the frame-layout calls, _timeline
 * and _destroy work unchanged.  WW_EINVAL before any state moves, ww_last_error naming the family to use instead: ww_stream_step,
 * _step_all, _step_trigger[_all], ww_pipeline_bank_step, ww_stream_feed* and ww_stream_set_model on a CTC bank; the three ww_*_ctc*
 * stream calls on any other bank.  Not offered: CTC members of model sets and every-member banks, feed, split-bf16, a fused
 * ww_pipeline_bank_step with this stage, more than WW_STREAM_CTC_MAX_LABELS labels per streamed window. */
#define WW_STREAM_CTC_STEPS 16u
#define WW_STREAM_CTC_MAX_LABELS 9
int ww_stream_create_ctc(ww_ctx *ctx, const ww_model *model, int32_t n_streams, const ww_frontend_params *fp, uint32_t flags,
                         ww_streams **out);
int ww_stream_step_ctc(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, int32_t max_labels, int32_t *labels,
                       int32_t *lengths, float *steps, int32_t *n_post);
int ww_ctc_trigger_bank_step(int32_t n_streams, const uint8_t *is_speech, uint8_t *is_active, const int32_t *labels,
                             const int32_t *lengths, const int32_t *n_post, int32_t max_labels, const int32_t *target,
                             int32_t n_target, uint8_t *was_speech, int32_t *fired_ids, int32_t *n_fired, int32_t *fall_ids,
                             int32_t *n_fall);
int ww_stream_step_ctc_trigger(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, uint8_t *is_active, int32_t max_labels,
                               const int32_t *target, int32_t n_target, uint8_t *was_speech, int32_t *labels, int32_t *lengths,
                               float *steps, int32_t *n_post, int32_t *fired_ids, int32_t *n_fired, int32_t *fall_ids, int32_t *n_fall);
/* ---- CTC stream banks: the forward-algorithm score per tick (ww_ctc_score_* above) ---------------------------------------------------
 * ww_stream_ctc_set_targets - gives a WW_STREAM_CTC_STEPS bank its targets and mode (ww_ctc_score_dev's arguments, T = 19, L = n_out;
 *   the same refusals); it may be called again between ticks.  WW_EINVAL on every other bank.
 * ww_stream_step_ctc_score - ww_stream_step_ctc plus ONE ctc_score_kernel launch behind the tick's model launch, on the same stream,
 *   over the bank's page-locked posterior block, into a page-locked [2 S][K]; scores [S][2][K] float32: window k of stream s, target j.
 *   Entries at or past n_post[s] are left as they were.  In every form of the bank (one launch, two launches, full recompute) a
 *   window's scores are the bits ww_ctc_score_dev gives on the posteriors the same tick returns in `steps` (which may be NULL).
 *   WW_EINVAL before any state moves on a bank without targets.  ww_stream_step_ctc on a bank with targets is what it was.
 * ww_ctc_score_trigger_bank_step - host only: ww_ctc_trigger_bank_step's VAD-edge bookkeeping, fired and fall lists with the score
 *   rule.  A stream that is not active fires on the first window of the tick on which some slot j has (double)score > thresholds[j]
 *   (ww_trigger_bank_step_all's comparison); fired_slot [n_fired] (may be NULL) names the exceeding slot with the greatest score on
 *   that window, the lowest slot among equals.  1 <= K <= WW_CTC_SCORE_MAX_TARGETS; WW_EINVAL with nothing touched otherwise. */
int ww_stream_ctc_set_targets(ww_streams *st, const int32_t *targets, const int32_t *target_lens, int32_t K, int32_t mode);
int ww_stream_step_ctc_score(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, int32_t max_labels, int32_t *labels,
                             int32_t *lengths, float *steps, float *scores, int32_t *n_post);
int ww_ctc_score_trigger_bank_step(int32_t n_streams, int32_t K, const uint8_t *is_speech, uint8_t *is_active, const float *scores,
                                   const int32_t *n_post, const double *thresholds, uint8_t *was_speech, int32_t *fired_ids,
                                   int32_t *fired_slot, int32_t *n_fired, int32_t *fall_ids, int32_t *n_fall);
/* ww_stream_step_ctc_align - ww_stream_step_ctc_score plus ONE ctc_align_kernel launch behind the score's, on the same posterior block:
 *   align_value [S][2][K] float32 and align_span [S][2][K][WW_CTC_SCORE_MAX_TARGET][2] int8 beside the scores (ww_ctc_align_* above, the
 *   bank's targets and mode), through a page-locked block the bank allocates on the first such call.  Entries at or past n_post[s] are
 *   left as they were.  In every form of the bank a window's alignment is the bits ww_ctc_align_dev gives on the posteriors the same
 *   tick returns in `steps`.  WW_EINVAL before any state moves: a bank without WW_STREAM_CTC_STEPS or without targets, a NULL output.
 *   ww_stream_step_ctc and ww_stream_step_ctc_score keep their launches. */
int ww_stream_step_ctc_align(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, int32_t max_labels, int32_t *labels,
                             int32_t *lengths, float *steps, float *scores, float *align_value, int8_t *align_span, int32_t *n_post);
/* ww_stream_step_ctc_beam - ww_stream_step_ctc plus ONE ctc_beam_kernel launch behind the tick's model launch, over the bank's
 *   page-locked posterior block (ww_ctc_beam_* above, T = 19, L = n_out): beam_labels [S][2][top_paths][beam_max_labels],
 *   beam_lengths [S][2][top_paths] and beam_probs [S][2][top_paths], through a page-locked block the bank allocates on the first such
 *   call.  Entries at or past n_post[s] are left as they were.  In every form of the bank a window's paths are the bits
 *   ww_ctc_beam_dev gives on the posteriors the same tick returns in `steps` (which may be NULL).  WW_EINVAL before any state moves:
 *   a bank without WW_STREAM_CTC_STEPS, beam_width / top_paths / beam_max_labels out of range, a NULL output.  The scores and the
 *   alignment are not carried in the same call. */
int ww_stream_step_ctc_beam(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, int32_t max_labels, int32_t *labels,
                            int32_t *lengths, float *steps, int32_t beam_width, int32_t top_paths, int32_t beam_max_labels,
                            int32_t *beam_labels, int32_t *beam_lengths, float *beam_probs, int32_t *n_post);
/* Where a tick's time goes on the HOST side of ww_stream_step(the loop of spokestack/pipeline.py:25-28 is host-paced, so
 * BASELINE config 5's per-tick latency is this call): mean nanoseconds per phase over the ticks since the last reset -
 * [0] plan (control words and window descriptors of the tick), [1] the caller's frames into the page-locked block,
 * [2] first kernel launch, [3] second kernel launch (0 where a tick is one launch), [4] waiting for the posteriors,
 * [5] copy-out into post / n_post.  A monotonic-clock read per phase: always on. */
#define WW_STREAM_TL_PHASES 6
int ww_stream_timeline(ww_streams *st, double *mean_ns, int64_t *ticks, int32_t reset);

/* ---- posterior smoothing + threshold sweep -----------------------------------------------
 * Replaces plot_FRR_FAR's numeric core (utils/evaluate_models.py:185-218):
 *   neg' = np.convolve(neg, ones(win)/win, 'same')   (fp64)
 *   frr[k] = (num_wakewords - #(pos > thr[k])) / num_wakewords
 *   fa_count[k] = #rising edges of (neg' > thr[k]);  fa_per_h[k] = fa_count[k] / hours
 * smoothed (may be NULL) receives neg' ([N] fp64).  win <= 0 skips the smoothing: neg' = (double)neg.
 *   positives   pos > thr[k] is a float32 comparison, pos[i] > (float)thr[k]: the reference pins numpy==1.19.5, where a float32
 *               array against a float64 scalar compares in float32.  A positive between thr[k] and (float)thr[k] is therefore
 *               judged by the rounded threshold.  The negatives' neg' > thr[k] is an fp64 comparison.
 *   thresholds  1 <= n_thr <= 1024, in any order, repeats allowed: entry k is counted against thr[k] alone.  n_thr > 1024 is
 *               WW_EINVAL and no output is written.
 *   NaN         a NaN is above nothing: a NaN positive is not accepted; a NaN row of neg makes the rows of neg' whose window holds it
 *               NaN, those rows are not above, and a run may begin on the row after them.
 * A negative stream shorter than win > 0 is refused (np.convolve 'same' would change its length). */
int ww_far_frr(ww_ctx *ctx, const float *pos, int64_t n_pos, const float *neg, int64_t n_neg, int32_t win,
               const double *thr, int32_t n_thr, double num_wakewords, double hours, double *frr,
               double *fa_per_h, int64_t *fa_count, double *smoothed);

/* The same sweep over posteriors that are already on the context's device (the sharded evaluators: the values a rank's
 * kernels produced, or what the posterior gather delivered) - d_pos / d_neg are device pointers, nothing but the thresholds goes
 * up and nothing but the n_thr counters comes back; d_smoothed (device, [n_neg] fp64) may be NULL.  Returns after the
 * counters are on the host.  Extent: nothing in front of or behind d_pos[0 .. n_pos) and d_neg[0 .. n_neg) reaches a counter or a
 * smoothed value (the window is clipped to the stream), and d_smoothed[0 .. n_neg) is written and nothing else. */
int ww_far_frr_dev(ww_ctx *ctx, const float *d_pos, int64_t n_pos, const float *d_neg, int64_t n_neg, int32_t win,
                   const double *thr, int32_t n_thr, double num_wakewords, double hours, double *frr, double *fa_per_h,
                   int64_t *fa_count, double *d_smoothed);

/* Posterior pick + per-clip reduction on the device (utils/evaluate_models.py:80,86: element [1] of a detect row - pidx per
 * SURVEY quirk C1 -; :98-99: the max over a wake-word clip's windows).  d_rows: [n][n_out] detect rows as the model entry points
 * leave them.  d_seg_offs == NULL: d_out[i] = d_rows[i][pidx] for all n rows (:105-106, the negative stream: every window
 * counts); otherwise d_seg_offs is a device table of n_seg + 1 ascending row offsets and d_out[s] = max over rows
 * [d_seg_offs[s], d_seg_offs[s + 1]).  Offsets are clamped to [0, n]; a run without rows yields -inf (the reference never asks
 * for one: np.max of nothing raises).  The maximum is np.max's: a run that holds a NaN yields NaN - such a clip is above no
 * threshold, as in the reference.  Enqueues on the context's stream, no synchronisation.
 * Extent: only element pidx of the rows of a run (of all n rows without a table) reaches d_out - not the other columns, not the
 * rows no run names, nothing around d_rows; d_out[0 .. n_seg) (or [0 .. n)) is written and nothing else. */
int ww_posterior_pick_dev(ww_ctx *ctx, const float *d_rows, int64_t n, int32_t n_out, int32_t pidx, const int64_t *d_seg_offs,
                          int64_t n_seg, float *d_out);

/* ---- detection events: WHERE the smoothed posterior is above the threshold -------------------
 * ww_far_frr counts the rising edges of (smoothed > threshold); these two calls say where they are - the library's counterpart of
 * the reference's examine_audio / plot_wav_and_posterior (utils/evaluate_models.py), for many recordings and many wake words at once.
 * Input
 *   post [planes][n] fp32, 1 <= planes <= 64 (one plane per wake word: ww_posterior_pick_dev makes them from detect rows)
 *   seg_offs [n_seg + 1]   ascending row offsets within [0, n], shared by all planes (HOST array); NULL = one segment [0, n).
 *                          Rows outside every segment belong to no event.
 *   win                    the smoothing window
 *   thr [planes] fp64      one threshold per plane (HOST array)
 * The rule, per plane k and segment u, p = the segment's m rows:
 *   sm[i]   the value ww_far_frr writes to smoothed[i] when given that segment alone as neg, bit for bit: the centre of the full
 *           convolution, sm[i] = sum over j = i + (win-1)/2 - (win-1) .. i + (win-1)/2, ascending, clipped to [0, m), of
 *           (double)p[j] * (1.0 / win), in fp64 (for m < win too, where ww_far_frr itself refuses the call); win <= 0: sm[i] =
 *           (double)p[i].  Smoothing never reads across a segment boundary.
 *   above   row i is above when sm[i] > thr[k], an fp64 compare: a NaN is not above (sweep_kernel's rule)
 *   event   a maximal run [start, end) of above rows inside the segment.  A run that reaches a segment's end ends there; a run that
 *           begins at the first row of the next segment is a new event.
 *   fields  start, end and peak are relative to the segment's first row; peak is the smallest i in the run at which sm is greatest,
 *           peak_value = sm[peak].
 * Order: by plane, then segment, then start; the output is identical from run to run (no atomics decide a position).
 * With one segment the number of events of plane k equals fa_count of ww_far_frr_dev on that plane at thr[k].
 * *n_events receives the total found; only the first min(total, cap) events in that order are written to `events`, nothing behind
 * them; events == NULL with cap == 0 counts only.  plane_counts (may be NULL) receives the total per plane.
 * WW_EINVAL with the reason in ww_last_error and no output written: planes outside 1..64; negative n, n_seg or cap; descending offsets
 * or offsets outside [0, n]; NULL thr or n_events; NULL events with cap > 0; NULL post with n > 0; more rows than one launch takes
 * (n > 2^39).  Both calls return with the events in the caller's array: ww_posterior_events_dev reads device posteriors where they
 * are - offsets and thresholds go up, the plane totals and the written events come back, nothing else crosses the bus -,
 * ww_posterior_events uploads host posteriors first.  Five kernel launches per call whatever n, n_seg, planes and the number of
 * events are (detection events).
 * Extent: the rows of a plane that no segment names, and what lies around d_post, reach no event, no peak value and no count; a
 * non-finite row affects the events of its own segment and plane alone. */
typedef struct ww_event {
  int32_t plane, seg;
  int64_t start, end, peak; /* segment-relative rows; the run is [start, end) */
  double peak_value;
} ww_event; /* 40 bytes */
int ww_posterior_events_dev(ww_ctx *ctx, const float *d_post, int64_t n, int32_t planes, const int64_t *seg_offs, int64_t n_seg,
                            int32_t win, const double *thr, ww_event *events, int64_t cap, int64_t *n_events, int64_t *plane_counts);
int ww_posterior_events(ww_ctx *ctx, const float *post, int64_t n, int32_t planes, const int64_t *seg_offs, int64_t n_seg, int32_t win,
                        const double *thr, ww_event *events, int64_t cap, int64_t *n_events, int64_t *plane_counts);

/* ---- superframe shortest-path smoothing -------------------------------------------------
 * Replaces wwdetect/wfst.py:17-71 `smooth()` (pynini 2-state x T lattice, tropical shortest path) as
 * wired in utils/CRNN_files/tflite.py:252-263 (superframe of 10 posteriors; trigger if the best path
 * visits 'wakeword').  in: [n][T][2] = (p_other, p_wakeword) per step, or -ln of them when in_is_cost != 0
 * (pass NumPy's -np.log for bit-exact reference costs).  stay_bonus = 1 in the reference.  path
 * (may be NULL) receives the best state sequence [n][T] (0 = other, 1 = wakeword), wake[n] = 1 if it
 * visits state 1.  T <= 64. */
int ww_superframe_smooth(ww_ctx *ctx, const float *in, int64_t n, int32_t T, float stay_bonus, int32_t in_is_cost,
                         uint8_t *path, uint8_t *wake);

#ifdef __cplusplus
}
#endif
#endif /* WWHIP_H */
