// Streaming mode: S concurrent 16 kHz streams advanced 20 ms per tick (BASELINE config 5).
//
// Device-resident replacement for the per-stream state of WakewordTrigger
// (spokestack/wakeword/tflite.py:92-108): sample ring, mel frame window, pre-emphasis carry.
// Per tick and stream the reference runs a 320-iteration Python loop that emits a frame
// whenever 512 samples are buffered and then drops the oldest 160 (tflite.py:163-168); with a
// ring that holds f <= 511 samples before the tick, that is exactly
//     n_frames = (f + 320 >= 512) ? (f + 320 - 512) / 160 + 1 : 0      (0, 1 or 2)
// frames at offsets 0, 160 of the concatenation [ring | new samples], and f' = f + 320 -
// 160 * n_frames samples kept.  The host mirrors f per stream (pure integer bookkeeping) so it
// knows the number of posteriors a tick will produce and can size the launch exactly; all
// sample and mel data stay in HBM.
//
// The front end's arithmetic and the mirrored ring's row store are stream_fe.h's, shared with the one-launch ticks of crnn.hip and
// wavenet.hip; the kernels here are
//   stream_frontend_kernel  one workgroup (2 waves) per stream: read the tick's samples and control words from
//                           pinned host memory, normalise + pre-emphasise the 320 new
//                           samples, FFT + mel for each new frame (one wave per frame) when
//                           the stream's is_speech bit is set, keep the ring tail.
//   The mel window of a stream is a MIRRORED ring of R = T + 1 slots (2R rows): row k of the stream's history is written at
//   k % R and at k % R + R, so the latest T rows up to row k are always the contiguous block [(k + 2) % R, +T) that the
//   model kernels' window descriptors want - two 160-byte stores per new frame instead of moving the whole 24-29 KB window
//   every tick (round 1's ping-pong shift).  The one spare slot is what lets BOTH windows of a two-frame tick be evaluated
//   after both rows are in place: the window that ends at row k leaves out exactly the slot of row k + 1.
//   then the regular CRNN / Wavenet kernels run on the compacted list of new windows.
//   stream_feed_frontend_kernel  a causal bank fed any number of samples per stream (ww_stream_feed, further down): one workgroup
//                           per 16 new frames of a stream, the same conversion and the same per-frame functions as above.
#include "model_set.h"  // (in front of fft_device.h's macros)
#include "stream_all.h"
#include "stream_ctc.h"
#include "ctc_score.h"
#include "ctc_align.h"
#include "ctc_beam.h"
#include "stream_fe.h"

#include <algorithm>
#include <sched.h>
#include <time.h>

#define ST_RING WW_ST_RING  // 511 + 320 rounded up
#define ST_WL_BYTES (((WW_MEL_TAPS * 64 * 4 + 2047) / 2048) * 2048)  // the mel weights in LDS, padded to whole rounds of 128 x 16 bytes

struct ww_streams {
  ww_ctx *ctx = nullptr;
  const ww_model *model = nullptr;
  int S = 0;
  ww_frontend_params fp = {};
  int T = 0, F = 0, NO = 0, HR = 0;  // HR = history rows per stream = 2 (T + 1) (mirrored ring)
  // device state
  float *ring = nullptr;      // [2][S][ST_RING] (the one-launch tick ping-pongs between the two copies by a stream's state parity; the
  float *hist = nullptr;      //  two-launch forms use the first) | [S][2 (T + 1)][F], mirrored ring
  float *prev = nullptr;      // [2][S] pre-emphasis carry (raw previous sample), likewise
  // per-tick device buffers
  int16_t *d_frames = nullptr;   // [S][320]
  int32_t *d_ctl = nullptr;      // [S][4]: fill, n_frames, flags, pos (history rows written so far, mod T + 1)
  int64_t *d_win_row = nullptr;  // [2S]
  int32_t *d_win_valid = nullptr;
  void *ws = nullptr;
  size_t ws_bytes = 0;           // capacity of ws (grown by ww_stream_step when the model's options ask for more)
  // host mirrors (pinned)
  int32_t *h_ctl = nullptr;
  int64_t *h_win_row = nullptr;
  int32_t *h_win_valid = nullptr;
  float *h_out = nullptr;
  float *h_out_dev = nullptr;   // the device's address of h_out
  int16_t *h_frames = nullptr;
  // the four per-tick inputs live in ONE pinned block (frames | win_row | ctl | win_valid) that the front-end kernel
  // reads over the bus itself - no copy-engine operation on a tick's path (four back-to-back host-to-device copies
  // cost 20 us of a 107 us tick); d_pack mirrors the layout and holds the window descriptors the kernel copies over.
  // The block exists TWICE (round 5): the one-launch tick alternates between the copies - a polled tick returns as soon as its
  // posteriors are in, while workgroups that owe none (a stream without a window only advances its ring) may not have read
  // their samples yet; by the time a copy is written again the kernel of the tick in between has started, i.e. this one ended
  char *h_pack = nullptr, *d_pack = nullptr, *h_pack_dev = nullptr;  // h_pack_dev: the device's address of h_pack
  size_t pack_bytes = 0;  // of ONE copy
  // a tick's posteriors as {value, tick number} pairs the model kernels store straight into page-locked memory (ww_tick_tag):
  // ww_stream_step polls them instead of waiting for the runtime's completion signal
  unsigned long long *h_tag = nullptr, *h_tag_dev = nullptr;  // [2 S]
  unsigned seq = 0;             // tick number (never 0 in a tag)
  unsigned flip = 0;            // which copy of the input block the tick at hand uses
  bool one_launch = false;      // incremental CRNN: front end inside the model kernel's workgroups (crnn_stream_kernel<1 | 2>)
  bool broken = false;          // a tick failed half way (ww_stream_step): no further ticks
  bool poll = false;            // wait by polling the tags (a context that owns its stream; WW_STREAM_SYNC_WAIT turns it off)
  std::vector<int> par;         // a stream's state parity (one-launch form)
  std::vector<int> expect;      // tag slots this tick's posteriors arrive in
  std::vector<int> fill, pos;
  // incremental CRNN (crnn.hip, crnn_stream_kernel): per-stream ring of projected interior rows, the row of an all-zero
  // field every slot holds after a reset, and the number of mel rows since the reset modulo the ring size
  float *gxc = nullptr, *gx_zero = nullptr;  // [S][WW_STREAM_GXC][192], [192]
  int32_t *h_win_aux = nullptr, *d_win_aux = nullptr;
  std::vector<int> rowq;
  bool incremental = false;
  // WW_STREAM_CAUSAL (fp32 Wavenet): the sequence form advanced row by row (wavenet.hip: wavenet_seq_kernel<1, stream>) - per stream
  // the blocks' last 16 rows of BatchNorm output, a ring of the last T logit rows, and {next ring slot, rows held}
  bool causal = false;
  float *wstate = nullptr, *zring = nullptr;  // [S][NB][WW_WAVE_STATE_BLOCK], [S][T][16]
  int32_t *zpos = nullptr;                    // [S][2]
  // host timeline of ww_stream_step (ww_stream_timeline): nanoseconds per phase summed over the ticks since the last reset
  uint64_t tl_ns[WW_STREAM_TL_PHASES] = {0};
  int64_t tl_ticks = 0;
  std::vector<uint8_t> stage_flags;  // ww_stream_step_trigger: bit 0 = is_speech, bit 1 = is_active per stream
  // a bank created from a model set (ww_stream_create_set): `model` is the set's view, stream s is served by member stream_model[s]
  // - the host's copy and the device table the SET kernels read -, and gx_zero holds one row per member
  const ww_model_set *set = nullptr;
  std::vector<int32_t> stream_model;
  int32_t *d_stream_model = nullptr;  // [S]
  ww_set_ref set_ref;                 // {d_stream_model, nullptr, the set's stride}
  // a bank at other rates than 16 kHz: ONE kernel of resample.hip in front of a tick's own turns the frames into the [S][320] block
  // the tick kernels read.  ww_stream_attach_resampler: frames are [S][frame samples of that rate] (a uniform bank);
  // ww_stream_attach_rates: one ragged block, stream s's frame at its own rate
  ww_stream_rates *rates = nullptr;
  int uniform_frame() const { return rates ? ww_k_rates_frame_samples(rates) : 0; }  // a uniform bank's frame samples; 0: not one
  bool g711() const { return rates && ww_k_rates_g711(rates); }  // some rate class reads G.711: frames and packets are counted in bytes
  bool used = false;                  // ticked or fed since creation
  // a bank that runs K member slots on every stream (ww_stream_create_set_all; stream_all.h): the model side - stream_model and its
  // device table, gxc, wstate, zring, zpos, h_tag, h_out, the window tables - is sized and indexed by VIRTUAL stream v = s K + slot,
  // the front-end side - ring, prev, hist, the control words, the frames - by physical stream.  Every other bank: K = 1, v = s
  int K = 1;
  bool every = false;
  std::vector<int32_t> members;       // [K] the member of each slot (an every-member bank)
  int V() const { return S * K; }
  // a CTC stream bank (ww_stream_create_ctc; stream_ctc.h): `model` is a CTC-trained CRNN, a tick's windows come back as decoded
  // labels - one 32-bit word per window in the tags or in h_out, which then holds words - and, on a WW_STREAM_CTC_STEPS bank, as
  // posteriors in h_steps [2 S][19][L].  The WW_STREAM_FULL_RECOMPUTE form runs ww_k_crnn_ctc_forward, whose labels [2 S][9] and
  // lengths [2 S] arrive in h_lab.  Everything else of the bank - rings, caches, tables, rates - is the ordinary bank's
  bool ctc = false, ctc_steps = false;
  float *h_steps = nullptr, *h_steps_dev = nullptr;
  int32_t *h_lab = nullptr, *h_lab_dev = nullptr;
  // ww_stream_ctc_set_targets (a WW_STREAM_CTC_STEPS bank): ww_stream_step_ctc_score runs ctc_score_kernel over h_steps behind the
  // tick's model launch, on the same stream; its scores arrive in h_score [2 S][K], slot for slot beside the posteriors
  bool score_set = false;
  ww_ctc_score_targets score_tg;
  float *h_score = nullptr, *h_score_dev = nullptr;
  // ww_stream_step_ctc_align: ctc_align_kernel over the same block with the same targets; one page-locked block, allocated by the
  // first such call: the values [2 S][WW_CTC_SCORE_MAX_TARGETS] float32, then the spans [2 S][WW_CTC_SCORE_MAX_TARGETS][9][2] int8
  // (a tick uses the first 2 S K of each)
  float *h_align = nullptr, *h_align_dev = nullptr;
  int8_t *h_span() const { return (int8_t *)(h_align + (size_t)2 * S * WW_CTC_SCORE_MAX_TARGETS); }
  int8_t *h_span_dev() const { return (int8_t *)(h_align_dev + (size_t)2 * S * WW_CTC_SCORE_MAX_TARGETS); }
  // ww_stream_step_ctc_beam: ctc_beam_kernel over the same posterior block; one page-locked block of 32-bit words, allocated by the
  // first such call for the widest call there is: labels [2 S][WW_CTC_BEAM_MAX_PATHS][19], then lengths and probabilities
  // [2 S][WW_CTC_BEAM_MAX_PATHS] each (a tick with P paths of M labels uses the first 2 S P M, 2 S P and 2 S P of them)
  int32_t *h_beam = nullptr, *h_beam_dev = nullptr;
  size_t beam_len_off() const { return (size_t)2 * S * WW_CTC_BEAM_MAX_PATHS * WW_SC_STEPS; }
  size_t beam_prob_off() const { return beam_len_off() + (size_t)2 * S * WW_CTC_BEAM_MAX_PATHS; }
  size_t beam_words() const { return beam_prob_off() + (size_t)2 * S * WW_CTC_BEAM_MAX_PATHS; }
  // the reason this bank refuses `call` (CTC or not: here; every-member or not: stream_all.h, sa_check_call), where ww_last_error
  // finds it; WW_OK: it does not
  int check_call(const char *call, bool wants_every, bool wants_ctc = false) const {
    if (ctc && !wants_ctc)
      return ww_fail(ctx, WW_EINVAL, "%s: this bank runs a CTC-trained CRNN (ww_stream_create_ctc), whose windows decode to labels: its tick is "
                     "ww_stream_step_ctc, its trigger stage ww_stream_step_ctc_trigger, and it has no posterior, no feed, no member and no fused pipeline step", call);
    if (!ctc && wants_ctc)
      return ww_fail(ctx, WW_EINVAL, "%s: this bank was not created by ww_stream_create_ctc: its tick is ww_stream_step and its family", call);
    char why[320];
    const int rc = sa_check_call(every, call, wants_every, why, sizeof why);
    return rc ? ww_fail(ctx, rc, "%s", why) : WW_OK;
  }
  // likewise the id list of a reset or a move (stream_all.h: sa_check_ids)
  int check_ids(const int32_t *ids, int32_t n) const {
    char why[64];
    const int rc = sa_check_ids(ids, n, S, why, sizeof why);
    return rc ? ww_fail(ctx, rc, "%s", why) : WW_OK;
  }
  // a call that failed after the host's mirrors (fill, ring positions, state parity, the member and rate tables) had moved leaves them
  // out of step with the device: `guarded` marks the bank, and `check_sound` refuses every later call that would build on them
  // instead of producing posteriors of a state that never existed
  int check_sound() const {
    return broken ? ww_fail(ctx, WW_ESTATE, "this stream bank failed in an earlier call: destroy it and create a new one") : WW_OK;
  }
  template <typename Body>
  int guarded(Body &&body) {  // body(bool *mutated): sets *mutated once the mirrors move
    bool mutated = false;
    const int rc = body(&mutated);
    if (rc != WW_OK && mutated) broken = true;
    return rc;
  }
  // the device's address of a place in the page-locked input block
  template <typename P>
  const P *dev_of(const P *host) const { return (const P *)(h_pack_dev + ((const char *)host - h_pack)); }
  // the kernels' extra argument: nullptr for a bank of one model
  const ww_set_ref *ref() const { return set ? &set_ref : nullptr; }
  int send_stream_model() {  // the host's copy -> the device table, in stream order (ww_tables::send, the one upload path)
    ww_tables tb;
    tb.add(stream_model);
    return tb.send(ctx, d_stream_model);
  }
};

static inline uint64_t st_now_ns() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

// scratch of the per-window kernels for nw windows (explicit window rows: never the sliding form)
static size_t model_scratch_bytes(const ww_model *m, int nw) {
  if (m->kind == WW_KIND_CRNN && m->crnn.HEAD == WW_HEAD_CTC) return ww_crnn_ctc_workspace(m, nw);
  return m->kind == WW_KIND_CRNN ? ww_crnn_workspace(m, nw, false) : ww_wave_workspace(m, nw);
}

struct stream_fe_args {
  const int16_t *frames;   // pinned host memory, read over the bus (640 B per stream and tick)
  const int32_t *ctl;      // pinned host memory
  const int64_t *h_row;    // pinned host: this tick's window rows / valid counts, copied to d_row / d_valid here
  const int32_t *h_valid;  //   for the model kernels that follow on the stream
  const int32_t *h_aux;    //   (+ the cache slots of the incremental CRNN kernel)
  int64_t *d_row;
  int32_t *d_valid, *d_aux;
  int nw, S;
  float *ring;
  float *hist;
  float *prev;
  int T, F, HR;
  ww_fe_pcm cv;
  int hop;
  ww_fe_filt fb;
};
// the kernel's dynamic LDS (bytes)
template <typename R>
struct stream_fe_lds {
  static constexpr size_t buf = 0;                                     // [2][FFT_LD] complex
  static constexpr size_t mag = buf + 2 * FFT_LD * sizeof(cplx<R>);    // [2][FE_MAG_LD]
  static constexpr size_t wl = mag + 2 * FE_MAG_LD * sizeof(float);    // the mel weights (rounded up to whole 128-thread store rounds)
  static constexpr size_t x = wl + ST_WL_BYTES;                        // [ST_RING] ring | new samples
  static constexpr size_t xs = x + ST_RING * sizeof(float);            // [WW_CHUNK] raw samples of the tick
  static constexpr size_t bytes = xs + WW_CHUNK * sizeof(short);
};

template <typename R>
__global__ __launch_bounds__(128) void stream_frontend_kernel(stream_fe_args a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x;
  // the tick's 320 samples (40 x 16 bytes) are requested from pinned host memory BEFORE the control words are looked at:
  // one trip over the bus instead of two in a row (control words -> branch -> samples)
  uint4 raw = make_uint4(0u, 0u, 0u, 0u);
  if (tid < 40) raw = ((const uint4 *)(a.frames + (size_t)s * WW_CHUNK))[tid];
  const int4 cw = ((const int4 *)a.ctl)[s];
  const int fill = cw.x, n_frames = cw.y, flags = cw.z, pos = cw.w;
  const bool speech = flags & 1, skip = flags & 2;

  typedef stream_fe_lds<R> L;
  cplx<R> *fbuf = (cplx<R> *)(smem + L::buf);
  float *mag = (float *)(smem + L::mag), *wl = (float *)(smem + L::wl), *x = (float *)(smem + L::x);
  short *xs = (short *)(smem + L::xs);

  // ---- this tick's window descriptors: host-pinned -> device arrays (read by the model kernels that follow).  A tick has at
  // most two windows per stream, i.e. one descriptor per thread of the first workgroups: requested here with everything else
  // that crosses the bus (unconditionally, from a clamped index), stored below once the loads behind them are out as well -
  // copied in place, the first workgroups waited for the bus before they asked for anything else
  const int di = s * 128 + tid, dic = di < a.nw ? di : 0;
  const int64_t h_row0 = a.h_row[dic];
  const int h_valid0 = a.h_valid[dic], h_aux0 = a.h_aux[dic];
  // device-side inputs that do not depend on the control words are requested before the branch on them, i.e. while
  // the control words and samples are still crossing the bus: mel weights, the whole sample ring (fill <= 511 of its
  // 832 slots are meaningful; the rest is never read), the pre-emphasis carry, the transform's constants
  constexpr int WLQ = ST_WL_BYTES / 16 / 128;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4 wlq[WLQ];
#pragma unroll
  for (int q = 0; q < WLQ; ++q) {
    const int i = tid + q * 128;
    wlq[q] = ((const f32x4 *)a.fb.wpad)[i < WW_MEL_TAPS * 64 / 4 ? i : 0];
  }
  const int mel_st = lane < a.fb.n_mel ? a.fb.start[lane] : 0;      // (the mel stage's two per-band scalars: asked for here, not
  const float mel_bias = lane < a.fb.n_mel ? a.fb.bias[lane] : 0.0f;  // behind the transform where they are used)
  float *ring = a.ring + (size_t)s * ST_RING;
  const float4 ringq = ((const float4 *)ring)[tid];  // samples 4 tid .. 4 tid + 3 (128 threads x 4 = 512 >= fill)
  const float carry = a.prev[s];
  fft_consts<R> fc;
  fft_load_consts<R>(fc, lane, a.fb.hann, a.fb.tw256, a.fb.tw512);
  // parked in LDS unconditionally and BEFORE the branch on the control words: behind it, and under a per-piece condition, the
  // compiler moved each load down to its store - five round trips to L2 in a row (the wl region is padded to whole rounds)
#pragma unroll
  for (int q = 0; q < WLQ; ++q) ((f32x4 *)wl)[tid + q * 128] = wlq[q];
  if (di < a.nw) {
    a.d_row[di] = h_row0;
    a.d_valid[di] = h_valid0;
    a.d_aux[di] = h_aux0;
  }
  for (int i = di + a.S * 128; i < a.nw; i += a.S * 128) {  // (more than 128 windows per stream and tick: not a shape the host produces)
    a.d_row[i] = a.h_row[i];
    a.d_valid[i] = a.h_valid[i];
    a.d_aux[i] = a.h_aux[i];
  }
  if (skip) return;  // context.is_active: the frame is not sampled at all (tflite.py:139-140)

  // ---- [ring | new samples] in LDS
  ((float4 *)x)[tid] = ringq;
  if (tid < 40) ((uint4 *)xs)[tid] = raw;
  __syncthreads();
  for (int i = tid; i < WW_CHUNK; i += 128) x[fill + i] = fe_sample(xs, i, carry, a.cv);
  __syncthreads();
  if (tid == 0) a.prev[s] = fe_norm(xs[WW_CHUNK - 1], a.cv);  // tflite.py:156-158: carry is the un-emphasised last sample
  // ---- new frames (wave k handles frame k); only analysed while is_speech (tflite.py:166)
  if (speech && wave < n_frames) {
    const float mv = fe_frame_mel<R>(x + wave * a.hop, fc, fbuf, mag, wave, wl, mel_st, mel_bias, a.fb, lane);
    if (lane < a.fb.n_mel) fe_ring_store(a.hist, (size_t)s * a.HR, pos + wave, a.T + 1, a.F, lane, mv);
  }
  __syncthreads();
  // ---- keep the ring tail
  const int keep = fill + WW_CHUNK - n_frames * a.hop;
  for (int i = tid; i < keep; i += 128) ring[i] = x[n_frames * a.hop + i];
}

// ---- a causal bank's feed (ww_stream_feed): the front end of any number of new samples per stream ---------------------------------
// One workgroup (4 waves) per group of up to FEED_GROUP new frames of one stream.  Frame f of a call covers samples
// [160 f, 160 f + 512) of [the stream's pending samples | the packet]; the group stages what its frames cover in LDS - the pending
// samples as they are, the packet's through the tick's conversion (fe_sample) - and each wave runs the tick's fe_frame_mel on its
// frames: a fed row is the tick's row bit for bit.
// The stream's state (pending samples, carry) is written by the stream's FIRST group (the only one when the packet completes no
// frame): pending samples are fewer than 512, so only frames 0..3 - the first group's - reach into them, and the carry belongs to
// the packet's first sample, which frame 0 covers.  The one reader being the one writer, the groups of a stream need no order.
#define FEED_WAVES 4
#define FEED_X (512 + (FEED_GROUP - 1) * 160)
// (FEED_GROUP and the tables feed_str - a stream of the call - and feed_grp: launch_plan.h)
struct feed_fe_args {
  const int16_t *pcm;
  const feed_str *str;
  const feed_grp *grp;
  float *rows;          // [rows of the call][F]
  float *ring, *hist, *prev;
  int T, F, HR;
  ww_fe_pcm cv;
  ww_fe_filt fb;
};
// the kernel's dynamic LDS (bytes)
template <typename R>
struct feed_fe_lds {
  static constexpr size_t buf = 0;                                              // [FEED_WAVES][FFT_LD] complex
  static constexpr size_t mag = buf + FEED_WAVES * FFT_LD * sizeof(cplx<R>);    // [FEED_WAVES][FE_MAG_LD]
  static constexpr size_t wl = mag + FEED_WAVES * FE_MAG_LD * sizeof(float);    // [WW_MEL_TAPS][64] the mel weights
  static constexpr size_t x = wl + WW_MEL_TAPS * 64 * sizeof(float);            // [FEED_X] what the group's frames cover
  static constexpr size_t pend = x + FEED_X * sizeof(float);                    // [512] the stream's new pending samples (first group)
  static constexpr size_t bytes = pend + 512 * sizeof(float);
};

template <typename R>
__global__ __launch_bounds__(FEED_WAVES * 64) void stream_feed_frontend_kernel(feed_fe_args a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const feed_grp g = a.grp[blockIdx.x];
  const feed_str d = a.str[g.i];
  const int s = d.sid, fill = d.fill;
  const bool first = g.f0 == 0;

  typedef feed_fe_lds<R> L;
  cplx<R> *fbuf = (cplx<R> *)(smem + L::buf);
  float *mag = (float *)(smem + L::mag), *wl = (float *)(smem + L::wl), *x = (float *)(smem + L::x), *pend = (float *)(smem + L::pend);

  for (int i = tid; i < WW_MEL_TAPS * 64 / 4; i += FEED_WAVES * 64) ((float4 *)wl)[i] = ((const float4 *)a.fb.wpad)[i];
  const int mel_st = lane < a.fb.n_mel ? a.fb.start[lane] : 0;
  const float mel_bias = lane < a.fb.n_mel ? a.fb.bias[lane] : 0.0f;
  float *ring = a.ring + (size_t)s * ST_RING;
  const int16_t *pk = a.pcm + d.s_off;
  const float carry = first ? a.prev[s] : 0.0f;  // (only the packet's first sample needs it, and only the first group covers that)
  fft_consts<R> fc;
  fft_load_consts<R>(fc, lane, a.fb.hann, a.fb.tw256, a.fb.tw512);
  // sample v of [pending | packet]
  auto sample = [&](int64_t v) -> float { return v < fill ? ring[v] : fe_sample(pk, v - fill, carry, a.cv); };
  const int64_t base = (int64_t)g.f0 * 160;
  const int len = g.nf > 0 ? (g.nf - 1) * 160 + 512 : 0;
  for (int i = tid; i < len; i += FEED_WAVES * 64) x[i] = sample(base + i);
  const int64_t tot = (int64_t)fill + d.k;
  const int keep = (int)(tot - (int64_t)d.rows * 160);  // < 512
  if (first)
    for (int i = tid; i < keep; i += FEED_WAVES * 64) pend[i] = sample((int64_t)d.rows * 160 + i);
  __syncthreads();  // x and pend complete; the ring and the carry have been read
  if (first) {
    for (int i = tid; i < keep; i += FEED_WAVES * 64) ring[i] = pend[i];
    if (tid == 0 && d.k > 0) a.prev[s] = fe_norm(pk[d.k - 1], a.cv);  // the un-emphasised last sample; an empty packet leaves the carry
  }
  // ---- the group's frames, wave k frames k, k + 4, ...: to the call's row buffer, the stream's last T + 1 rows also into its
  //      mirrored ring (row r of the call at slot (pos + r) % (T + 1), as the ticks would have left them)
  const int slots = a.T + 1;
  const int ring_from = d.rows > slots ? d.rows - slots : 0;
  for (int fl = wave; fl < g.nf; fl += FEED_WAVES) {
    const float mv = fe_frame_mel<R>(x + fl * 160, fc, fbuf, mag, wave, wl, mel_st, mel_bias, a.fb, lane);
    const int r = g.f0 + fl;
    if (lane < a.fb.n_mel) {
      a.rows[(size_t)(d.r_off + r) * a.F + lane] = mv;
      // (a call can bring more rows than the ring has slots: reduced below `slots` here)
      if (r >= ring_from) fe_ring_store(a.hist, (size_t)s * a.HR, (int)(((int64_t)d.pos + r) % slots), slots, a.F, lane, mv);
    }
    wave_sync();  // the wave is through with its magnitudes before the next frame's transform writes them
  }
}

// a causal bank's reset: the next row is row 0 of a new sequence (zero history, empty ring; the ring's rows need no clearing)
__global__ void stream_causal_reset_kernel(float *wstate, int32_t *zpos, const int32_t *ids, int S, int state_floats) {
  const int b = blockIdx.x;
  const int s = ids ? ids[b] : b;
  if (s < 0 || s >= S) return;
  for (int i = threadIdx.x; i < state_floats; i += blockDim.x) wstate[(size_t)s * state_floats + i] = 0.f;
  if (threadIdx.x < 2) zpos[2 * s + threadIdx.x] = 0;
}

// gx_zero: [192], or with stream_model (a bank of a model set) [members][192]: the row of the stream's current member
__global__ void stream_reset_kernel(float *hist, const int32_t *ids, int S, int HR, int F, float *gxc, const float *gx_zero,
                                    const int32_t *stream_model) {
  const int b = blockIdx.x;
  const int s = ids ? ids[b] : b;
  if (s < 0 || s >= S) return;
  for (int i = threadIdx.x; i < HR * F; i += blockDim.x) hist[(size_t)s * HR * F + i] = 0.f;
  if (gxc) {  // every cached row = the row of an all-zero field (what lies in front of the stream's first mel rows)
    float *c = gxc + (size_t)s * WW_STREAM_GXC * 192;
    const float *z = gx_zero + (stream_model ? (size_t)stream_model[s] * 192 : 0);
    for (int i = threadIdx.x; i < WW_STREAM_GXC * 192; i += blockDim.x) c[i] = z[i % 192];
  }
}

// The reset's kernels for `count` streams (d_ids == nullptr: streams 0 .. count - 1).  A bank of K member slots per stream resets a
// stream's front end once and its K model states: the mel history by physical id, then the caches by virtual id (d_vids: the count K
// virtual streams of d_ids; nullptr with d_ids: all) - stream_reset_kernel with zero history rows touches the caches alone.
static void stream_reset_launch(ww_streams *st, const int32_t *d_ids, const int32_t *d_vids, int count) {
  ww_ctx *ctx = st->ctx;
  const int K = st->K;
  if (K == 1) {
    hipLaunchKernelGGL(stream_reset_kernel, dim3(count), dim3(256), 0, ctx->stream, st->hist, d_ids, st->S, st->HR, st->F, st->gxc,
                       (const float *)st->gx_zero, (const int32_t *)st->d_stream_model);
  } else {
    hipLaunchKernelGGL(stream_reset_kernel, dim3(count), dim3(256), 0, ctx->stream, st->hist, d_ids, st->S, st->HR, st->F, (float *)nullptr,
                       (const float *)nullptr, (const int32_t *)nullptr);
    if (st->gxc)
      hipLaunchKernelGGL(stream_reset_kernel, dim3(count * K), dim3(256), 0, ctx->stream, st->hist, d_vids, st->V(), 0, st->F, st->gxc,
                         (const float *)st->gx_zero, (const int32_t *)st->d_stream_model);
  }
  if (st->causal)
    hipLaunchKernelGGL(stream_causal_reset_kernel, dim3(count * K), dim3(256), 0, ctx->stream, st->wstate, st->zpos, K == 1 ? d_ids : d_vids,
                       st->V(), (int)st->model->wave.dil.size() * WW_WAVE_STATE_BLOCK);
}

extern "C" {

int ww_stream_destroy(ww_streams *st) {
  WW_GUARD_BEGIN
  if (!st) return WW_OK;
  ww_device_scope dev_scope(st->ctx->device);
  hipStreamSynchronize(st->ctx->stream);
  void *dev[] = {st->ring, st->hist, st->prev, st->d_pack, st->ws, st->gxc, st->gx_zero, st->wstate, st->zring, st->zpos, st->d_stream_model};
  for (void *p : dev)
    if (p) hipFree(p);
  void *host[] = {st->h_pack, st->h_out, st->h_tag, st->h_steps, st->h_lab, st->h_score, st->h_align, st->h_beam};
  for (void *p : host)
    if (p) hipHostFree(p);
  ww_k_rates_destroy(st->rates);
  delete st;
  return WW_OK;
  WW_GUARD_END(nullptr)
}

}  // extern "C"

// ww_stream_create (set == nullptr), ww_stream_create_set (model = the set's view; stream_model: checked by the caller, or nullptr) and
// ww_stream_create_set_all (every_k > 0: stream_model = the every_k member slots, checked by the caller, or nullptr);
// ww_stream_create_ctc (ctc: the model is a CTC-trained CRNN, checked by the caller; flags may carry WW_STREAM_CTC_STEPS)
static int stream_create_impl(ww_ctx *ctx, const ww_model *model, const ww_model_set *set, const int32_t *stream_model, int32_t S,
                              const ww_frontend_params *fp, uint32_t flags, ww_streams **out, int every_k = 0, bool ctc = false) {
  if (!ctc)
    if (int rc = ww_crnn_refuse_ctc(ctx, model, "ww_stream_create")) return rc;
  const bool ctc_steps = ctc && (flags & WW_STREAM_CTC_STEPS);
  if (ctc) flags &= ~(uint32_t)WW_STREAM_CTC_STEPS;
  if (flags & ~(uint32_t)(WW_STREAM_FULL_RECOMPUTE | WW_STREAM_TWO_LAUNCH | WW_STREAM_SYNC_WAIT | WW_STREAM_CAUSAL))
    return ww_fail(ctx, WW_EINVAL, "unknown stream flags 0x%x", flags);
  const bool causal = (flags & WW_STREAM_CAUSAL) != 0;
  if (causal && (flags & WW_STREAM_FULL_RECOMPUTE))
    return ww_fail(ctx, WW_EINVAL, "WW_STREAM_CAUSAL advances cached activations: it cannot be combined with WW_STREAM_FULL_RECOMPUTE");
  if (causal && (model->kind != WW_KIND_WAVENET || model->precision != WW_PRECISION_FP32))
    return ww_fail(ctx, WW_EINVAL, "WW_STREAM_CAUSAL is the fp32 Wavenet's sequence form: not for a CRNN or a model in split-bf16 mode");
  if (S <= 0 || S > 65535) return ww_fail(ctx, WW_EINVAL, "stream count %d out of range (1..65535)", S);
  if (fp->hop != 160) return ww_fail(ctx, WW_EINVAL, "streaming mode supports hop 160 (10 ms @ 16 kHz) only, got %d", fp->hop);
  if (!(fp->pcm_divisor > 0.f)) return ww_fail(ctx, WW_EINVAL, "pcm_divisor must be positive");
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  ww_streams *st = new ww_streams();
  ww_scoped<ww_streams, ww_stream_destroy> own(st);  // (freed on every early return below)
  st->ctx = ctx; st->model = model; st->S = S; st->fp = *fp;
  st->ctc = ctc; st->ctc_steps = ctc_steps;
  if (every_k) {
    st->every = true;
    st->K = every_k;
    sa_member_table(stream_model, every_k, 1, st->members);
  }
  const int V = st->V();
  if (set) {
    st->set = set;
    if (every_k) sa_member_table(stream_model, every_k, S, st->stream_model);
    else if (stream_model) st->stream_model.assign(stream_model, stream_model + S);
    else st->stream_model.assign((size_t)S, 0);
    if (hipMalloc((void **)&st->d_stream_model, ww_bump::need((size_t)V, 4)) != hipSuccess)
      return ww_fail(ctx, WW_ENOMEM, "cannot allocate the model table of %d streams", V);
    st->set_ref.ids = st->d_stream_model;
    st->set_ref.stride = (long long)set->stride;
  }
  st->T = model->info.window; st->F = model->info.n_mel; st->NO = model->info.n_out; st->HR = 2 * (st->T + 1);
  const size_t hist_elems = (size_t)S * st->HR * st->F;
  // CRNN, standard geometry: three positions per new window instead of nineteen (crnn_stream_kernel, fp32 contractions - also
  // for a model in split-bf16 mode: a seventh of the products in fp32 is both faster and closer).
  // WW_STREAM_FULL_RECOMPUTE keeps the per-window kernels (every window recomputed from its mel rows).
  st->incremental = ww_crnn_stream_capable(model) && !(flags & WW_STREAM_FULL_RECOMPUTE);
  // ONE launch per tick: the incremental CRNN at any size (tools/stream_forms.py: 7 % faster from 128 to 1,024 streams), the
  // Wavenet while a tick's windows stay within its twelve-wave form (ww_wave_tick_capable: up to 128 streams)
  st->causal = causal;  // (always the front-end kernel + one model kernel)
  // (an every-member Wavenet bank always runs in two launches)
  st->one_launch = !causal && !(flags & WW_STREAM_TWO_LAUNCH) &&
                   ((st->incremental && model->filt.n_mel == 40) || (!every_k && ww_wave_tick_capable(model, S)));
  // a borrowed stream is the caller's: when the call returns everything enqueued on it has completed, as before
  st->poll = ctx->own_stream && !(flags & WW_STREAM_SYNC_WAIT);
  // (stream_ctc.h: no order is built between a window's posteriors and its tag, so a bank that returns posteriors waits for the stream)
  if (ctc_steps) st->poll = false;
  // model scratch of the per-window kernels; the incremental CRNN needs none
  size_t ws_bytes = st->incremental ? 256 : model_scratch_bytes(model, 2 * V);
  bool ok = hipMalloc((void **)&st->ring, (size_t)2 * S * ST_RING * 4) == hipSuccess &&
            hipMalloc((void **)&st->hist, hist_elems * 4) == hipSuccess &&
            hipMalloc((void **)&st->prev, (size_t)2 * S * 4) == hipSuccess &&
            hipMalloc(&st->ws, ws_bytes) == hipSuccess && ((st->ws_bytes = ws_bytes), true) &&
            hipHostMalloc((void **)&st->h_out, (size_t)2 * V * st->NO * 4) == hipSuccess &&
            hipHostMalloc((void **)&st->h_tag, (size_t)2 * V * 8) == hipSuccess;
  {
    const size_t o_frames = 0, o_row = o_frames + (size_t)S * WW_CHUNK * 2, o_ctl = o_row + (size_t)2 * V * 8,
                 o_valid = o_ctl + (size_t)S * 16, o_aux = o_valid + (size_t)2 * V * 4;
    st->pack_bytes = o_aux + (size_t)2 * V * 4;
    st->pack_bytes = (st->pack_bytes + 255) & ~(size_t)255;
    ok = ok && hipMalloc((void **)&st->d_pack, st->pack_bytes) == hipSuccess &&
         hipHostMalloc((void **)&st->h_pack, 2 * st->pack_bytes) == hipSuccess;
    if (ok) {
      st->h_frames = (int16_t *)(st->h_pack + o_frames); st->d_frames = (int16_t *)(st->d_pack + o_frames);
      st->h_win_row = (int64_t *)(st->h_pack + o_row);   st->d_win_row = (int64_t *)(st->d_pack + o_row);
      st->h_ctl = (int32_t *)(st->h_pack + o_ctl);       st->d_ctl = (int32_t *)(st->d_pack + o_ctl);
      st->h_win_valid = (int32_t *)(st->h_pack + o_valid); st->d_win_valid = (int32_t *)(st->d_pack + o_valid);
      st->h_win_aux = (int32_t *)(st->h_pack + o_aux);     st->d_win_aux = (int32_t *)(st->d_pack + o_aux);
    }
  }
  if (ctc) {
    ok = ok && (!ctc_steps || hipHostMalloc((void **)&st->h_steps, (size_t)2 * S * WW_SC_STEPS * st->NO * 4) == hipSuccess) &&
         (st->incremental || hipHostMalloc((void **)&st->h_lab, (size_t)2 * S * (WW_STREAM_CTC_MAX_LABELS + 1) * 4) == hipSuccess);
    if (ok && st->h_steps && hipHostGetDevicePointer((void **)&st->h_steps_dev, st->h_steps, 0) != hipSuccess) ok = false;
    if (ok && st->h_lab && hipHostGetDevicePointer((void **)&st->h_lab_dev, st->h_lab, 0) != hipSuccess) ok = false;
  }
  if (!ok) {
    return ww_fail(ctx, WW_ENOMEM, "cannot allocate state for %d streams", S);
  }
  memset(st->h_tag, 0, (size_t)2 * V * 8);
  if (hipHostGetDevicePointer((void **)&st->h_out_dev, st->h_out, 0) != hipSuccess ||
      hipHostGetDevicePointer((void **)&st->h_tag_dev, st->h_tag, 0) != hipSuccess ||
      hipHostGetDevicePointer((void **)&st->h_pack_dev, st->h_pack, 0) != hipSuccess) {
    return ww_fail(ctx, WW_EHIP, "pinned staging buffers are not visible to the device");
  }
  hipMemsetAsync(st->ring, 0, (size_t)2 * S * ST_RING * 4, ctx->stream);
  hipMemsetAsync(st->hist, 0, hist_elems * 4, ctx->stream);
  hipMemsetAsync(st->prev, 0, (size_t)2 * S * 4, ctx->stream);
  hipMemsetAsync(st->d_pack, 0, st->pack_bytes, ctx->stream);
  memset(st->h_pack, 0, 2 * st->pack_bytes);
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  st->fill.assign(S, 0);
  st->pos.assign(S, 0);
  st->rowq.assign(S, 0);
  st->par.assign(S, 0);
  st->expect.reserve((size_t)2 * V);
  if (st->incremental) {
    const int K = set ? set->n : 1;  // gx_zero is a function of the weights: one row per member
    if (hipMalloc((void **)&st->gxc, (size_t)V * WW_STREAM_GXC * 192 * 4) != hipSuccess ||
        hipMalloc((void **)&st->gx_zero, (size_t)K * 192 * 4) != hipSuccess) {
      return ww_fail(ctx, WW_ENOMEM, "cannot allocate the projected-row cache of %d streams", V);
    }
    // the row of an all-zero field: position 17 of one window over the (all-zero) history of stream 0, which the kernel
    // stores into slot (0 + 128) % ring of stream 0's cache.  A set: once per member, stream 0 lent to each in turn
    std::vector<int32_t> real;
    if (set) real.swap(st->stream_model);
    for (int k = 0; k < K; ++k) {
      if (set) {
        st->stream_model.assign((size_t)V, k);
        if (int rc = st->send_stream_model()) return rc;
      }
      hipMemsetAsync(st->gxc, 0, (size_t)WW_STREAM_GXC * 192 * 4, ctx->stream);
      // d_pack is zeroed: window row 0, aux 0 (valid 0 = all-zero window)
      int rc = ctc ? ww_k_crnn_ctc_stream_forward(ctx, model, st->hist, (int64_t)S * st->HR, st->d_win_row, st->d_win_valid, st->d_win_aux, st->gxc, 1,
                                                  (uint32_t *)st->h_out_dev, nullptr)
                   : ww_k_crnn_stream_forward(ctx, model, st->hist, (int64_t)S * st->HR, st->d_win_row, st->d_win_valid, st->d_win_aux,
                                              st->gxc, 1, st->h_out_dev, nullptr, st->ref());
      if (rc) {
        return rc;
      }
      hipMemcpyAsync(st->gx_zero + (size_t)k * 192, st->gxc + (size_t)(128 % WW_STREAM_GXC) * 192, 192 * 4, hipMemcpyDeviceToDevice, ctx->stream);
    }
    if (set) {
      st->stream_model.swap(real);
      if (int rc = st->send_stream_model()) return rc;
    }
    stream_reset_launch(st, nullptr, nullptr, S);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess) {
      return ww_fail(ctx, WW_EHIP, "streaming CRNN set-up failed");
    }
  }
  if (causal) {
    const size_t b_state = (size_t)V * (int)model->wave.dil.size() * WW_WAVE_STATE_BLOCK * 4, b_ring = (size_t)V * st->T * 16 * 4;
    if (hipMalloc((void **)&st->wstate, b_state) != hipSuccess || hipMalloc((void **)&st->zring, b_ring) != hipSuccess ||
        hipMalloc((void **)&st->zpos, (size_t)V * 2 * 4) != hipSuccess)
      return ww_fail(ctx, WW_ENOMEM, "cannot allocate the causal state of %d streams", V);
    hipMemsetAsync(st->wstate, 0, b_state, ctx->stream);
    hipMemsetAsync(st->zring, 0, b_ring, ctx->stream);
    hipMemsetAsync(st->zpos, 0, (size_t)V * 2 * 4, ctx->stream);
    WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (set && !st->incremental) {  // (the incremental bank sent it above, behind its members' turns)
    if (int rc = st->send_stream_model()) return rc;
    WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  *out = own.release();
  return WW_OK;
}

extern "C" {

int ww_stream_create(ww_ctx *ctx, const ww_model *model, int32_t S, const ww_frontend_params *fp, uint32_t flags,
                     ww_streams **out) {
  WW_GUARD_BEGIN
  if (!ctx || !model || !fp || !out) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  *out = nullptr;
  return stream_create_impl(ctx, model, nullptr, nullptr, S, fp, flags, out);
  WW_GUARD_END(ctx)
}

int ww_stream_create_set(ww_ctx *ctx, const ww_model_set *set, int32_t S, const int32_t *stream_model, const ww_frontend_params *fp,
                         uint32_t flags, ww_streams **out) {
  WW_GUARD_BEGIN
  if (!ctx || !set || !fp || !out) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  *out = nullptr;
  if (set->ctx != ctx) return ww_fail(ctx, WW_EINVAL, "the model set belongs to another context");
  if (flags & WW_STREAM_FULL_RECOMPUTE)
    return ww_fail(ctx, WW_EINVAL, "WW_STREAM_FULL_RECOMPUTE runs the per-window batch kernels: not offered on a model set");
  if (set->view.kind == WW_KIND_CRNN && !ww_crnn_stream_capable(&set->view))
    return ww_fail(ctx, WW_EINVAL, "a CRNN set streams through the incremental kernel: standard conv geometry only");
  if (S > 0) {
    char why[160];
    if (int rc = ww_set_check_ids(stream_model, S, set->n, "stream_model", why, sizeof why)) return ww_fail(ctx, rc, "ww_stream_create_set: %s", why);
  }
  return stream_create_impl(ctx, &set->view, set, stream_model, S, fp, flags, out);
  WW_GUARD_END(ctx)
}

// Every listed member on every stream (include/wwhip.h; stream_all.h): the set bank of n_streams x n_members virtual streams
int ww_stream_create_set_all(ww_ctx *ctx, const ww_model_set *set, int32_t S, const int32_t *members, int32_t n_members,
                             const ww_frontend_params *fp, uint32_t flags, ww_streams **out) {
  WW_GUARD_BEGIN
  if (!ctx || !set || !fp || !out) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  *out = nullptr;
  if (set->ctx != ctx) return ww_fail(ctx, WW_EINVAL, "the model set belongs to another context");
  if (!members) n_members = set->n;
  char why[320];
  if (int rc = sa_check_create(S, n_members, flags, why, sizeof why)) return ww_fail(ctx, rc, "ww_stream_create_set_all: %s", why);
  if (set->view.kind == WW_KIND_CRNN && !ww_crnn_stream_capable(&set->view))
    return ww_fail(ctx, WW_EINVAL, "a CRNN set streams through the incremental kernel: standard conv geometry only");
  if (int rc = ww_set_check_ids(members, n_members, set->n, "members", why, sizeof why)) return ww_fail(ctx, rc, "ww_stream_create_set_all: %s", why);
  return stream_create_impl(ctx, &set->view, set, members, S, fp, flags, out, n_members);
  WW_GUARD_END(ctx)
}

// The bank becomes one at the resampler's input rate (include/wwhip.h).  The refusals that depend on the rates and the state object
// are ww_k_rates_create's (resample.hip; stream_rate.h): the bank of ONE resampling class with every stream in it for good (a uniform
// bank); no kernel of the bank changes, a tick only reads its samples elsewhere.
static int attach_resampler_impl(ww_streams *st, const ww_resampler *r, const int32_t *format, const char *what) {
  ww_ctx *ctx = st->ctx;
  if (!r) return ww_fail(ctx, WW_EINVAL, "%s: NULL resampler", what);
  if (int rc = st->check_sound()) return rc;
  if (st->uniform_frame()) return ww_fail(ctx, WW_EINVAL, "%s: this bank already has a resampler (%d Hz frames)", what, st->uniform_frame() * 50);
  if (st->rates) return ww_fail(ctx, WW_EINVAL, "%s: this bank already has per-stream rates (ww_stream_attach_rates)", what);
  if (st->used) return ww_fail(ctx, WW_ESTATE, "%s: the bank has ticked or been fed: a resampler is attached to a new bank", what);
  WW_ON_DEVICE(ctx, dev_scope);
  return ww_k_rates_create(ctx, &r, format, 1, nullptr, st->S, true, what, &st->rates);
}

int ww_stream_attach_resampler(ww_streams *st, const ww_resampler *r) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  return attach_resampler_impl(st, r, nullptr, "ww_stream_attach_resampler");
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// ww_stream_attach_resampler for frames and packets of in_format (include/wwhip.h): the uniform bank, [S][F] of the format
int ww_stream_attach_resampler_fmt(ww_streams *st, const ww_resampler *r, int32_t in_format) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  return attach_resampler_impl(st, r, &in_format, "ww_stream_attach_resampler_fmt");
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// A bank whose stream s runs at the input rate of class stream_rate[s] (include/wwhip.h).  What depends on the classes and the state
// object are ww_k_rates_create's (resample.hip; stream_rates.h); no kernel of the bank changes, a tick only reads its samples elsewhere.
static int attach_rates_impl(ww_streams *st, const ww_resampler *const *rs, const int32_t *formats, int32_t n_rates, const int32_t *stream_rate,
                             const char *what) {
  ww_ctx *ctx = st->ctx;
  if (!rs) return ww_fail(ctx, WW_EINVAL, "%s: NULL class table", what);
  if (int rc = st->check_sound()) return rc;
  if (n_rates < 1 || n_rates > WW_STREAM_MAX_RATES) return ww_fail(ctx, WW_EINVAL, "%s: %d rate classes: a bank has 1..%d", what, (int)n_rates, WW_STREAM_MAX_RATES);
  if (st->uniform_frame()) return ww_fail(ctx, WW_EINVAL, "%s: this bank already has a resampler (%d Hz frames)", what, st->uniform_frame() * 50);
  if (st->rates) return ww_fail(ctx, WW_EINVAL, "%s: this bank already has its rates (%d classes)", what, ww_k_rates_classes(st->rates));
  if (st->used) return ww_fail(ctx, WW_ESTATE, "%s: the bank has ticked or been fed: rates are attached to a new bank", what);
  WW_ON_DEVICE(ctx, dev_scope);
  return ww_k_rates_create(ctx, rs, formats, n_rates, stream_rate, st->S, false, what, &st->rates);
}

int ww_stream_attach_rates(ww_streams *st, const ww_resampler *const *rs, int32_t n_rates, const int32_t *stream_rate) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  return attach_rates_impl(st, rs, nullptr, n_rates, stream_rate, "ww_stream_attach_rates");
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// ww_stream_attach_rates where class k reads its frames and packets as formats[k] (include/wwhip.h): a class is a (rate, format) pair
// (stream_formats.h).  formats == NULL: ww_stream_attach_rates itself.
int ww_stream_attach_rates_fmt(ww_streams *st, const ww_resampler *const *rs, const int32_t *formats, int32_t n_rates, const int32_t *stream_rate) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  if (!formats) return attach_rates_impl(st, rs, nullptr, n_rates, stream_rate, "ww_stream_attach_rates");
  return attach_rates_impl(st, rs, formats, n_rates, stream_rate, "ww_stream_attach_rates_fmt");
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// A plain bank's frames (no rates attached): WW_CHUNK int16 samples per stream, back to back.  `unit`: 1 counts samples, 2 bytes.
static void plain_layout(int S, int unit, int32_t *frame, int64_t *offs) {
  for (int s = 0; s <= S; ++s) {
    if (s < S) frame[s] = WW_CHUNK * unit;
    offs[s] = (int64_t)s * WW_CHUNK * unit;
  }
}

int ww_stream_frame_layout(const ww_streams *st, int32_t *frame_samples, int64_t *frame_offs) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  if (!frame_samples || !frame_offs) return ww_fail(st->ctx, WW_EINVAL, "ww_stream_frame_layout: NULL argument");
  if (st->g711())
    return ww_fail(st->ctx, WW_EINVAL, "ww_stream_frame_layout: this bank has G.711 streams, its frames are counted in bytes: ww_stream_frame_layout_bytes");
  if (st->rates) ww_k_rates_layout(st->rates, frame_samples, frame_offs);
  else plain_layout(st->S, 1, frame_samples, frame_offs);
  return WW_OK;
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// The listed streams move to another rate class of the bank and start afresh: the table first, then ww_stream_reset's kernels behind
// it on the stream, exactly as ww_stream_set_model does.
int ww_stream_set_rate(ww_streams *st, const int32_t *ids, int32_t n, int32_t rate_class) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  ww_ctx *ctx = st->ctx;
  if (!st->rates || st->uniform_frame()) return ww_fail(ctx, WW_EINVAL, "ww_stream_set_rate: this bank has no per-stream rates (ww_stream_attach_rates)");
  if (int rc = st->check_sound()) return rc;
  const int K = ww_k_rates_classes(st->rates);
  if (rate_class < 0 || rate_class >= K) return ww_fail(ctx, WW_EINVAL, "ww_stream_set_rate: class %d: the bank has rate classes 0..%d", (int)rate_class, K - 1);
  if (int rc = st->check_ids(ids, n)) return rc;
  const int count = ids ? n : st->S;
  if (count == 0) return WW_OK;
  WW_ON_DEVICE(ctx, dev_scope);
  return st->guarded([&](bool *mutated) {
    *mutated = true;  // (a failed upload may or may not have been enqueued: which table the device holds is not known)
    if (int rc = ww_k_rates_move(st->rates, ids, count, rate_class)) return rc;
    return ww_stream_reset(st, ids, n);
  });
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// The byte layout of a tick's frames on any bank (include/wwhip.h; stream_formats.h: formats_layout)
int ww_stream_frame_layout_bytes(const ww_streams *st, int32_t *frame_bytes, int64_t *byte_offs, int32_t *formats) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  if (!frame_bytes || !byte_offs || !formats) return ww_fail(st->ctx, WW_EINVAL, "ww_stream_frame_layout_bytes: NULL argument");
  if (st->rates) {
    ww_k_rates_layout_bytes(st->rates, frame_bytes, byte_offs, formats);
  } else {
    plain_layout(st->S, 2, frame_bytes, byte_offs);
    std::fill(formats, formats + st->S, (int32_t)WW_SAMPLE_I16);
  }
  return WW_OK;
  WW_GUARD_END(st ? st->ctx : nullptr)
}

int ww_stream_frame_samples(const ww_streams *st, int32_t *out) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  if (!out) return ww_fail(st->ctx, WW_EINVAL, "ww_stream_frame_samples: NULL argument");
  if (st->g711())
    return ww_fail(st->ctx, WW_EINVAL, "ww_stream_frame_samples: this bank has G.711 streams, its frames are counted in bytes: ww_stream_frame_layout_bytes");
  if (st->rates && !st->uniform_frame())
    return ww_fail(st->ctx, WW_EINVAL, "ww_stream_frame_samples: the streams of this bank have frames of their own: ww_stream_frame_layout");
  *out = st->rates ? st->uniform_frame() : WW_CHUNK;
  return WW_OK;
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// The listed streams move to another member of the bank's set and start afresh: the table first, then ww_stream_reset's kernels
// behind it on the stream (they read the new member's gx_zero row).
int ww_stream_set_model(ww_streams *st, const int32_t *ids, int32_t n, int32_t model) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  ww_ctx *ctx = st->ctx;
  if (int rc = st->check_call("ww_stream_set_model", false)) return rc;  // (an every-member bank has a set: no refusal changes places)
  if (!st->set) return ww_fail(ctx, WW_EINVAL, "ww_stream_set_model: this bank was not created from a model set");
  if (int rc = st->check_sound()) return rc;
  if (model < 0 || model >= st->set->n) return ww_fail(ctx, WW_EINVAL, "ww_stream_set_model: model %d: the set has members 0..%d", (int)model, st->set->n - 1);
  if (int rc = st->check_ids(ids, n)) return rc;
  const int count = ids ? n : st->S;
  if (count == 0) return WW_OK;
  WW_ON_DEVICE(ctx, dev_scope);
  // the host's table is what the device's was last sent: it changes only with an upload that was enqueued (a failed one may or may
  // not have been: which table the device holds is not known), and a failure behind that point (the reset's kernels) leaves streams
  // on their new member with their old caches: no further ticks
  return st->guarded([&](bool *mutated) {
    *mutated = true;
    const std::vector<int32_t> before = st->stream_model;
    for (int i = 0; i < count; ++i) st->stream_model[ids ? ids[i] : i] = model;
    if (int rc = st->send_stream_model()) {
      st->stream_model = before;
      return rc;
    }
    return ww_stream_reset(st, ids, n);
  });
  WW_GUARD_END(st ? st->ctx : nullptr)
}

int ww_stream_reset(ww_streams *st, const int32_t *ids, int32_t n) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  ww_ctx *ctx = st->ctx;
  if (int rc = st->check_ids(ids, n)) return rc;
  const int count = ids ? n : st->S;
  if (count == 0) return WW_OK;
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  int32_t *d_ids = nullptr, *d_vids = nullptr;
  if (ids) {
    // reuse the window-valid buffer (2 S ints: sa_check_ids's bound) as id staging
    memcpy(st->h_win_valid, ids, (size_t)n * 4);
    WW_HIP(ctx, hipMemcpyAsync(st->d_win_valid, st->h_win_valid, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    d_ids = st->d_win_valid;
    if (st->K > 1) {  // the K virtual streams of each: staged in the aux table (2 S K ints as well)
      std::vector<int32_t> vids;
      sa_virtual_ids(ids, n, st->K, vids);
      memcpy(st->h_win_aux, vids.data(), vids.size() * 4);
      WW_HIP(ctx, hipMemcpyAsync(st->d_win_aux, st->h_win_aux, vids.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      d_vids = st->d_win_aux;
    }
  }
  stream_reset_launch(st, d_ids, d_vids, count);
  WW_HIP(ctx, hipGetLastError());
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // WakewordTrigger.reset (tflite.py:241-246): sample window emptied, frame window zeroed;
  // _prev_sample is NOT reset by the reference and is not reset here.
  for (int i = 0; i < count; ++i) {
    const int s = ids ? ids[i] : i;
    st->fill[s] = 0;
    st->pos[s] = 0;
    st->rowq[s] = 0;
  }
  if (st->rates) ww_k_rates_reset(st->rates, ids, count);  // the next sample is x[0] of a new signal: D zeros lead again
  return WW_OK;
  WW_GUARD_END(st ? st->ctx : nullptr)
}

int ww_stream_window(ww_streams *st, int32_t stream, float *out) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  ww_ctx *ctx = st->ctx;
  if (!out) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (stream < 0 || stream >= st->S) return ww_fail(ctx, WW_EINVAL, "stream id %d out of range", stream);
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  // the T rows that end at the last row written (pos - 1) start at slot (pos - 1 + 2) % R of the mirrored ring.  Copied behind
  // everything enqueued so far (a polled tick returns once its posteriors are in, while workgroups that owe none may still be
  // writing rows), then waited for
  const int R = st->T + 1;
  const float *src = st->hist + ((size_t)stream * st->HR + (st->pos[stream] + 1) % R) * st->F;
  WW_HIP(ctx, hipMemcpyAsync(out, src, (size_t)st->T * st->F * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return WW_OK;
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// Wait for a tick's posteriors by polling their {value, tick number} pairs in page-locked memory.  The runtime is asked only
// now and then whether the stream has drained (a kernel that died would otherwise leave the host spinning for ever).
// A tick that has not delivered after WW_TICK_TIMEOUT_S seconds (a kernel that neither finishes nor fails: a hung GPU) is an error
// as well - the caller gets WW_EHIP and a bank that refuses further ticks instead of a host thread that spins for ever.
#ifndef WW_TICK_TIMEOUT_S
#define WW_TICK_TIMEOUT_S 10
#endif
static int st_poll_tags(ww_streams *st) {
  ww_ctx *ctx = st->ctx;
  const size_t n = st->expect.size();
  const unsigned seq = st->seq;
  size_t i = 0;
  unsigned spins = 0;
  uint64_t t_slow = 0;  // when the wait left the fast path (first runtime query)
  while (i < n) {
    const unsigned long long v = __atomic_load_n(st->h_tag + st->expect[i], __ATOMIC_ACQUIRE);
    if ((unsigned)(v >> 32) == seq) {
      ++i;
      continue;
    }
    __builtin_ia32_pause();
    if (spins > (1u << 18)) sched_yield();  // (a tick that is milliseconds late - a GPU busy elsewhere - stops pinning the core)
    if ((++spins & 0x3fffu) == 0) {
      const hipError_t q = hipStreamQuery(ctx->stream);
      if (q == hipErrorNotReady) {
        const uint64_t now = st_now_ns();
        if (!t_slow) t_slow = now;
        if (now - t_slow > (uint64_t)WW_TICK_TIMEOUT_S * 1000000000ull)
          return ww_fail(ctx, WW_EHIP, "streaming tick %u did not complete within %d s (posterior slot %d still missing)", seq, WW_TICK_TIMEOUT_S,
                         st->expect[i]);
        continue;
      }
      if (q != hipSuccess) return ww_fail(ctx, WW_EHIP, "streaming tick failed: %s", hipGetErrorString(q));
      for (size_t r = i; r < n; ++r)  // the stream has drained: what will ever arrive has
        if ((unsigned)(__atomic_load_n(st->h_tag + st->expect[r], __ATOMIC_ACQUIRE) >> 32) != seq)
          return ww_fail(ctx, WW_EHIP, "streaming tick %u completed without delivering posterior slot %d", seq, st->expect[r]);
      break;
    }
  }
  return WW_OK;
}

// where a CTC bank's tick puts what it decoded (ww_stream_step_ctc's arguments, checked there)
struct st_ctc_out {
  int max_labels;
  int32_t *labels, *lengths;  // [S][2][max_labels], [S][2]
  float *steps;               // [S][2][19][L] or nullptr
  float *scores;              // [S][2][K] or nullptr (ww_stream_step_ctc_score: the bank's targets are set)
  float *align_value = nullptr;  // [S][2][K] and [S][2][K][9][2], or nullptr (ww_stream_step_ctc_align)
  int8_t *align_span = nullptr;
  // ww_stream_step_ctc_beam: [S][2][P][M], [S][2][P], [S][2][P], or nullptr
  int beam_width = 0, top_paths = 0, beam_max_labels = 0;
  int32_t *beam_labels = nullptr, *beam_lengths = nullptr;
  float *beam_probs = nullptr;
};

// The one tick of every bank.  co (a CTC bank, stream_ctc.h): the same bookkeeping, frames, front end and wait; the model launches
// are the CTC forms', and what arrives is scattered as labels, lengths and posteriors instead of `post` (nullptr then).
static int stream_step_impl(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, float *post, int32_t *n_post, bool *mutated,
                            const st_ctc_out *co = nullptr) {
  ww_ctx *ctx = st->ctx;
  if (!frames || !is_speech || (!post && !co) || !n_post) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  *mutated = true;  // from here on the host's mirrors of the streams' state advance
  st->used = true;
  const int S = st->S, hop = st->fp.hop;
  uint64_t tl[WW_STREAM_TL_PHASES + 1];
  tl[0] = st_now_ns();
  if (++st->seq == 0) st->seq = 1;  // (a tag of tick 0 is "never written")
  // which copy of the page-locked input block this tick uses (the one-launch form alternates, see ww_streams)
  st->flip ^= 1u;  // (a bit of its own: the tick number skips 0 when it wraps)
  const size_t cp = st->one_launch ? (size_t)st->flip * st->pack_bytes : 0;
  int16_t *h_frames = (int16_t *)((char *)st->h_frames + cp);
  int32_t *h_ctl = (int32_t *)((char *)st->h_ctl + cp);
  st->expect.clear();
  // the tick's bookkeeping, control words, descriptors and tag slots: stream_all.h, per physical stream for its K virtual ones
  sa_tick tk;
  tk.S = S; tk.K = st->K; tk.T = st->T; tk.HR = st->HR;
  tk.hop = hop; tk.chunk = WW_CHUNK; tk.window = WW_FFT_WINDOW; tk.gxc = WW_STREAM_GXC;
  tk.form = st->one_launch ? SA_ONE_LAUNCH : st->causal ? SA_CAUSAL : SA_TABLE;
  tk.fill = st->fill.data(); tk.pos = st->pos.data(); tk.rowq = st->rowq.data(); tk.par = st->par.data();
  tk.ctl = h_ctl; tk.row = st->h_win_row; tk.valid = st->h_win_valid; tk.aux = st->h_win_aux;
  tk.expect = &st->expect;
  for (int s = 0; s < S; ++s) n_post[s] = sa_tick_stream(tk, s, is_speech[s]);
  const int nw = tk.nw, nw_c = tk.nd;  // windows of the tick | causal: virtual streams with new rows
  tl[1] = st_now_ns();
  // a bank at other rates: its frames go through ww_k_rates_tick's kernel into a device block, and the tick reads that
  const int16_t *rate_frames = nullptr;
  if (st->rates) {
    if (int rc = ww_k_rates_tick(st->rates, frames, is_speech, st->dev_of(h_ctl), &rate_frames)) return rc;
  } else {
    memcpy(h_frames, frames, (size_t)S * WW_CHUNK * 2);
  }
  tl[2] = st_now_ns();
  const ww_model *m = st->model;
  // posterior element: width-1 head -> [0]; width-2 head -> [1]  
  const int pidx = st->NO == 1 ? 0 : 1;
  ww_tick_tag tag = {st->h_tag_dev, st->seq, pidx};
  bool tagged = false;
  bool second = false;  // a second kernel was launched behind the tick's first
  if (st->one_launch) {
    // ---- ONE launch: front end + model, workgroup 2 v + k = window k of (virtual) stream v (crnn.hip: crnn_stream_kernel<FE>; wavenet.hip)
    ww_tick_fe fe = {};
    fe.frames = rate_frames ? rate_frames : st->dev_of(h_frames);
    fe.ctl = st->dev_of(h_ctl);
    fe.ring = st->ring; fe.prev = st->prev; fe.hist = st->hist;
    fe.S = S; fe.HR = st->HR;
    fe.cv = ww_fe_pcm_of(st->fp); fe.hop = hop;
    int rc = co ? ww_k_crnn_ctc_tick(ctx, m, fe, st->fp.precise, st->gxc, tag, st->h_steps_dev)
             : m->kind == WW_KIND_CRNN ? ww_k_crnn_tick(ctx, m, fe, st->fp.precise, st->gxc, tag, st->ref(), st->every ? st->K : 0) : ww_k_wave_tick(ctx, m, fe, st->fp.precise, tag, st->ref());
    if (rc) return rc;
    tagged = true;
    tl[3] = st_now_ns();
  } else {
    stream_fe_args a = {};
    // no copy engine on the tick's path: the kernel reads the pinned staging block itself
    a.frames = rate_frames ? rate_frames : st->dev_of(st->h_frames);
    a.ctl = st->dev_of(st->h_ctl);
    a.h_row = st->dev_of(st->h_win_row);
    a.h_valid = st->dev_of(st->h_win_valid);
    a.h_aux = st->dev_of(st->h_win_aux);
    a.d_row = st->d_win_row; a.d_valid = st->d_win_valid; a.d_aux = st->d_win_aux; a.nw = st->causal ? nw_c : nw; a.S = S;
    a.ring = st->ring;
    a.hist = st->hist; a.prev = st->prev;
    a.T = st->T; a.F = st->F; a.HR = st->HR;
    a.cv = ww_fe_pcm_of(st->fp); a.hop = hop;
    a.fb = ww_fe_filt_of(m->filt);
    {
      ww_launch_scope scope(ctx, "stream_frontend_kernel");
      if (st->fp.precise)
        hipLaunchKernelGGL((stream_frontend_kernel<double>), dim3(S), dim3(128), stream_fe_lds<double>::bytes, ctx->stream, a);
      else
        hipLaunchKernelGGL((stream_frontend_kernel<float>), dim3(S), dim3(128), stream_fe_lds<float>::bytes, ctx->stream, a);
    }
    WW_HIP(ctx, hipGetLastError());
    tl[3] = st_now_ns();
    if (st->causal) {
      // the model kernel of a causal tick: one workgroup per stream with new rows; posteriors land in slot 2 s + k.  Polled only
      // when the tick owes a posterior (a tick that owes none still has to see its front end through before the next one
      // rewrites the page-locked block)
      tagged = st->poll && !st->expect.empty();
      int rc = ww_k_wave_stream_tick(ctx, m, st->hist, st->d_win_row, st->d_win_valid, st->d_win_aux, nw_c, st->wstate, st->zring, st->zpos,
                                     st->h_out_dev, tagged ? &tag : nullptr, st->ref());
      if (rc) return rc;
      second = nw_c > 0;
    } else if (nw && !st->incremental) {
      // the per-window kernels' scratch under the model's options of THIS tick (ww_model_set_option may have lowered the
      // front/tail threshold since the bank was created: the split form then wants nw x 19 x 192 floats)
      const size_t need = model_scratch_bytes(m, nw);
      if (need > st->ws_bytes) {
        WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
        WW_HIP(ctx, hipFree(st->ws));
        st->ws = nullptr;
        st->ws_bytes = 0;
        const size_t want = model_scratch_bytes(m, 2 * st->V());
        if (hipMalloc(&st->ws, want > need ? want : need) != hipSuccess) return ww_fail(ctx, WW_ENOMEM, "cannot grow the model scratch of %d streams", S);
        st->ws_bytes = want > need ? want : need;
      }
    }
    if (nw && !st->causal) {
      // the heads store a tick's few posteriors straight into pinned host memory - as {value, tick number} pairs where the
      // launch form writes them (every one-kernel form), else as rows of h_out: no device-to-host copy (a DMA operation of
      // its own) between the last kernel and the host's wake-up
      // (a CTC bank: the incremental kernel writes tags; the full-recompute form's tail writes labels and lengths, never tags)
      tagged = st->poll && (st->incremental || (!co && (m->kind == WW_KIND_WAVENET || ww_crnn_forward_tags(m, nw))));
      const ww_tick_tag *tg = tagged ? &tag : nullptr;
      const float *d_hist = st->hist;
      // (a set's two-launch Wavenet tick: the kernel finds its stream in the window's aux word, which it has no other use for)
      ww_set_ref wref = st->set_ref;
      wref.aux = st->d_win_aux;
      const ww_set_ref *wset = st->set ? &wref : nullptr;
      int rc = co ? (st->incremental
                         ? ww_k_crnn_ctc_stream_forward(ctx, m, d_hist, (int64_t)S * st->HR, st->d_win_row, st->d_win_valid, st->d_win_aux, st->gxc, nw,
                                                        (uint32_t *)st->h_out_dev, st->h_steps_dev, tg)
                         : ww_k_crnn_ctc_forward(ctx, m, d_hist, (int64_t)S * st->HR, st->d_win_row, st->d_win_valid, 0, 0, 0, nw, st->ws, st->ws_bytes,
                                                 WW_STREAM_CTC_MAX_LABELS, st->h_lab_dev, st->h_lab_dev + (size_t)2 * S * WW_STREAM_CTC_MAX_LABELS,
                                                 st->h_steps_dev, nullptr))
               : st->incremental
                   ? ww_k_crnn_stream_forward(ctx, m, d_hist, (int64_t)S * st->HR, st->d_win_row, st->d_win_valid, st->d_win_aux, st->gxc, nw, st->h_out_dev, tg, st->ref())
               : m->kind == WW_KIND_CRNN
                   ? ww_k_crnn_forward(ctx, m, d_hist, (int64_t)S * st->HR, st->d_win_row, st->d_win_valid, 0, 0, 0, nw, st->ws, st->ws_bytes, st->h_out_dev, nullptr, tg)
                   : ww_k_wave_forward(ctx, m, d_hist, (int64_t)S * st->HR, st->d_win_row, st->d_win_valid, 0, 0, 0, nw, st->ws, st->ws_bytes, st->h_out_dev, nullptr, tg, wset);
      if (rc) return rc;
      second = true;
    }
  }
  // ww_stream_step_ctc_score: the forward-algorithm scores of the tick's windows, one more launch behind the model's, over the
  // posterior block slot for slot (the table form fills slots 0 .. nw - 1, the one-launch form slot 2 s + k: all 2 S are scored, and a
  // slot no window of this tick wrote is not read back)
  if (co && co->scores && nw)
    if (int rc = ww_k_ctc_score(ctx, st->h_steps_dev, tk.form == SA_TABLE ? nw : 2 * S, WW_SC_STEPS, st->NO, st->score_tg, st->h_score_dev, 1, st->score_tg.K))
      return rc;
  // ww_stream_step_ctc_align: and the alignment of the same slots, one launch more
  if (co && co->align_value && nw)
    if (int rc = ww_k_ctc_align(ctx, st->h_steps_dev, tk.form == SA_TABLE ? nw : 2 * S, WW_SC_STEPS, st->NO, st->score_tg, st->h_align_dev,
                                st->h_span_dev(), 1, st->score_tg.K))
      return rc;
  // ww_stream_step_ctc_beam: the beam search over the same slots, one launch behind the model's
  if (co && co->beam_labels && nw)
    if (int rc = ww_k_ctc_beam(ctx, st->h_steps_dev, tk.form == SA_TABLE ? nw : 2 * S, WW_SC_STEPS, st->NO, co->beam_width, co->top_paths, co->beam_max_labels,
                               st->h_beam_dev, st->h_beam_dev + st->beam_len_off(), (float *)(st->h_beam_dev + st->beam_prob_off())))
      return rc;
  // (include/wwhip.h: phase [3] is 0 where a tick is one launch - the one-launch forms, and a two-launch bank's tick without a window:
  // no clock read of its own, which on a tick's first pass through this code measured the branches above, not a launch)
  tl[4] = second ? st_now_ns() : tl[3];
  if (tagged && st->poll && nw) {
    int rc = st_poll_tags(st);
    if (rc) return rc;
  } else {
    WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  tl[5] = st_now_ns();
  if (co) {
    // labels / lengths [s][k] from where the window's word arrived (stream_ctc.h): a tag's low word, a word of h_out, or - the
    // full-recompute form - the tail's own labels and length; the posteriors from the same slot of h_steps
    const bool table = tk.form == SA_TABLE;
    sc_scatter(table, S, n_post, [&](int slot) -> uint32_t {
      if (!st->incremental)
        return ww_sc_pack(st->h_lab + (size_t)slot * WW_STREAM_CTC_MAX_LABELS, st->h_lab[(size_t)2 * S * WW_STREAM_CTC_MAX_LABELS + slot]);
      return tagged ? (uint32_t)st->h_tag[slot] : ((const uint32_t *)st->h_out)[slot];
    }, co->max_labels, co->labels, co->lengths);
    if (co->steps) {
      const size_t row = (size_t)WW_SC_STEPS * st->NO;
      int w = 0;
      for (int s = 0; s < S; ++s)
        for (int k = 0; k < n_post[s]; ++k, ++w)
          memcpy(co->steps + ((size_t)s * 2 + k) * row, st->h_steps + (size_t)(table ? w : 2 * s + k) * row, row * sizeof(float));
    }
    if (co->scores) {
      const size_t row = (size_t)st->score_tg.K;
      int w = 0;
      for (int s = 0; s < S; ++s)
        for (int k = 0; k < n_post[s]; ++k, ++w)
          memcpy(co->scores + ((size_t)s * 2 + k) * row, st->h_score + (size_t)(table ? w : 2 * s + k) * row, row * sizeof(float));
    }
    if (co->align_value) {
      const size_t row = (size_t)st->score_tg.K, srow = row * 2 * WW_CTC_SCORE_MAX_TARGET;
      int w = 0;
      for (int s = 0; s < S; ++s)
        for (int k = 0; k < n_post[s]; ++k, ++w) {
          const size_t slot = (size_t)(table ? w : 2 * s + k);
          memcpy(co->align_value + ((size_t)s * 2 + k) * row, st->h_align + slot * row, row * sizeof(float));
          memcpy(co->align_span + ((size_t)s * 2 + k) * srow, st->h_span() + slot * srow, srow);
        }
    }
    if (co->beam_labels) {
      const size_t P = (size_t)co->top_paths, lrow = P * co->beam_max_labels;
      int w = 0;
      for (int s = 0; s < S; ++s)
        for (int k = 0; k < n_post[s]; ++k, ++w) {
          const size_t slot = (size_t)(table ? w : 2 * s + k), o = (size_t)s * 2 + k;
          memcpy(co->beam_labels + o * lrow, st->h_beam + slot * lrow, lrow * 4);
          memcpy(co->beam_lengths + o * P, st->h_beam + st->beam_len_off() + slot * P, P * 4);
          memcpy(co->beam_probs + o * P, st->h_beam + st->beam_prob_off() + slot * P, P * 4);
        }
    }
  } else
  // post[s][slot][k] from where it arrived (stream_all.h): a tag's low word, or the posterior column of a row of h_out
  sa_scatter(tk.form, S, st->K, n_post, [&](int slot) -> float {
    if (!tagged) return st->h_out[(size_t)slot * st->NO + pidx];
    const unsigned bits = (unsigned)st->h_tag[slot];
    float p;
    memcpy(&p, &bits, 4);
    return p;
  }, post);
  tl[6] = st_now_ns();
  for (int i = 0; i < WW_STREAM_TL_PHASES; ++i) st->tl_ns[i] += tl[i + 1] - tl[i];
  ++st->tl_ticks;
  return WW_OK;
}

// ww_stream_step, ww_stream_step_all and (co: a CTC bank's outputs) ww_stream_step_ctc: the refusals, then the one tick
static int stream_step_entry(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, float *post, int32_t *n_post, const char *call,
                             bool wants_every, const st_ctc_out *co = nullptr) {
  if (int rc = st->check_call(call, wants_every, co != nullptr)) return rc;
  if (int rc = st->check_sound()) return rc;
  return st->guarded([&](bool *mutated) { return stream_step_impl(st, frames, is_speech, post, n_post, mutated, co); });
}

int ww_stream_step(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, float *post, int32_t *n_post) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  return stream_step_entry(st, frames, is_speech, post, n_post, "ww_stream_step", false);
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// The tick of an every-member bank (include/wwhip.h): ww_stream_step's body, post [S][K][2]
int ww_stream_step_all(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, float *post, int32_t *n_post) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  return stream_step_entry(st, frames, is_speech, post, n_post, "ww_stream_step_all", true);
  WW_GUARD_END(st ? st->ctx : nullptr)
}

int ww_stream_members(const ww_streams *st, int32_t *members, int32_t *n_members) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  if (!n_members) return ww_fail(st->ctx, WW_EINVAL, "ww_stream_members: NULL argument");
  *n_members = st->every ? st->K : 0;
  if (members)
    for (int j = 0; st->every && j < st->K; ++j) members[j] = st->members[(size_t)j];
  return WW_OK;
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// ---- ww_stream_feed: a causal bank advanced by any subset of its streams and any number of samples for each --------------------
// The framing is the tick's rule for k samples instead of 320: tot = fill + k, rows = tot >= 512 ? (tot - 512) / 160 + 1 : 0,
// fill' = tot - 160 rows.  Everything a refusal can depend on is looked at here, before any state moves.
// A bank at other rates: k is what the packet's samples come to at 16 kHz (ww_k_rates_advance), and offs16 (n + 1 entries, from 0)
// receives the sample_offs the rest of the feed then works with.
// all: the call is an every-member bank's (ww_stream_feed_all, ww_stream_feed_rows_all) - row_offs counts mel rows all the same, and
// a call's rows x K posteriors have the bound a call's rows have.
static int feed_check(ww_streams *st, const int32_t *ids, int32_t n, const int64_t *sample_offs, int64_t *row_offs, const char *what,
                      std::vector<int64_t> *offs16 = nullptr, bool all = false) {
  ww_ctx *ctx = st->ctx;
  if (int rc = st->check_call(what, all)) return rc;
  if (!st->causal) return ww_fail(ctx, WW_EINVAL, "%s: only a bank created with WW_STREAM_CAUSAL can be fed (a window bank recomputes a window per row)", what);
  if (int rc = st->check_sound()) return rc;
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "%s: negative stream count", what);
  if (!sample_offs || !row_offs || (n > 0 && !ids)) return ww_fail(ctx, WW_EINVAL, "%s: NULL argument", what);
  std::vector<uint8_t> seen((size_t)st->S, 0);
  std::vector<int64_t> offs((size_t)n + 1, 0);  // row_offs is written once nothing can refuse the call any more
  int64_t rows = 0;
  if (offs16) offs16->assign((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) {
    const int s = ids[i];
    if (s < 0 || s >= st->S) return ww_fail(ctx, WW_EINVAL, "%s: stream id %d out of range", what, s);
    if (seen[s]) return ww_fail(ctx, WW_EINVAL, "%s: stream %d is named twice", what, s);
    seen[s] = 1;
    int64_t k = sample_offs[i + 1] - sample_offs[i];
    if (k < 0) return ww_fail(ctx, WW_EINVAL, "%s: sample_offs descend at entry %d", what, i);
    if (st->rates) k = ww_k_rates_advance(st->rates, s, k);
    if (offs16) (*offs16)[(size_t)i + 1] = (*offs16)[(size_t)i] + k;
    const int64_t r = ww_fe_frames(st->fill[s] + k, st->fp.hop);
    if (r > 0x3fffffff || rows + r > 0x3fffffff) return ww_fail(ctx, WW_EINVAL, "%s: more than 2^30 rows in one call", what);
    rows += r;
    if (all && rows * st->K > 0x3fffffff)
      return ww_fail(ctx, WW_EINVAL, "%s: more than 2^30 posteriors (rows x %d member slots) in one call", what, st->K);
    offs[(size_t)i + 1] = rows;
  }
  memcpy(row_offs, offs.data(), offs.size() * 8);
  return WW_OK;
}

int ww_stream_feed_rows(ww_streams *st, const int32_t *ids, int32_t n, const int64_t *sample_offs, int64_t *row_offs) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  return feed_check(st, ids, n, sample_offs, row_offs, "ww_stream_feed_rows");
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// ww_stream_feed, and ww_stream_feed_all (all: a bank of K member slots per stream, stream_all.h).  The plan, the uploaded samples, the
// front end and the host's mirrors are the PHYSICAL streams' and run once whatever K is; the model side - the sequence kernel's
// every-member form, the tail's tables, the logits and posteriors - is the virtual streams' v = s K + slot.
// byte_offs (ww_stream_feed_bytes on a bank with G.711 streams): packet i is bytes [byte_offs[i], byte_offs[i + 1]) of pcm in its
// stream's format, and sample_offs counts its samples; nullptr: pcm is int16 and packet i is its samples [sample_offs[i], sample_offs[i + 1]).
static int stream_feed_impl(ww_streams *st, const int32_t *ids, int32_t n, const int16_t *pcm, const int64_t *sample_offs, int64_t cap_rows,
                            int64_t *row_offs, float *post, float *mel, bool *mutated, bool all = false, const int64_t *byte_offs = nullptr,
                            const char *what = nullptr) {
  ww_ctx *ctx = st->ctx;
  if (!what) what = all ? "ww_stream_feed_all" : "ww_stream_feed";
  std::vector<int64_t> offs16, offs_out((size_t)(n > 0 ? n : 0) + 1, 0);
  // (the caller's row_offs is written when no refusal is left)
  if (int rc = feed_check(st, ids, n, sample_offs, sample_offs && row_offs ? offs_out.data() : nullptr, what, &offs16, all)) return rc;
  const int64_t rows = offs_out[(size_t)n], samples_in = n > 0 ? sample_offs[n] - sample_offs[0] : 0;
  if (cap_rows < rows) return ww_fail(ctx, WW_EINVAL, "%s: the call produces %lld rows, the buffers hold %lld", what, (long long)rows, (long long)cap_rows);
  if (samples_in > 0 && !pcm) return ww_fail(ctx, WW_EINVAL, "%s: NULL sample buffer", what);
  if (rows > 0 && !post) return ww_fail(ctx, WW_EINVAL, "%s: NULL posterior buffer", what);
  memcpy(row_offs, offs_out.data(), offs_out.size() * 8);
  if (samples_in == 0) return WW_OK;  // nothing arrived: no stream moves
  st->used = true;
  // a bank at other rates: from here on the packets are their 16 kHz samples, which ww_k_rates_feed leaves on the device
  const int64_t *in_offs = sample_offs;
  if (st->rates) sample_offs = offs16.data();
  const int64_t samples = sample_offs[n] - sample_offs[0];
  const ww_model *m = st->model;
  const int T = st->T, F = st->F, NO = st->NO, R = T + 1, hop = st->fp.hop, rf = ww_wave_receptive_field(m);
  const int K = st->K;  // (1 unless `all`)
  if ((size_t)(WW_FEED_POOL_ROWS + T - 1) * 64 > 64 * 1024) return ww_fail(ctx, WW_EINVAL, "%s: windows of up to %d rows only", what, 1024 - WW_FEED_POOL_ROWS + 1);
  WW_ON_DEVICE(ctx, dev_scope);
  feed_plan pl;  // launch_plan.h
  feed_make_plan(ids, n, sample_offs, row_offs, st->fill.data(), st->pos.data(), T, rf, m->opt_wave_seq_segment, pl);
  if (all) feed_plan_all(pl, K, rows);
  const std::vector<feed_grp> &grp = pl.grp;
  const std::vector<wv_feed_seg> &small = pl.small, &large = pl.large;
  if (grp.size() > 0x7fffffffu || small.size() + large.size() > 0x7fffffffu || pl.pool.size() > 0x7fffffffu)
    return ww_fail(ctx, WW_EINVAL, "%s: too much work for one call", what);
  // ---- the call's scratch: [tables | samples | mel rows | logits | posteriors] in the context's workspace
  ww_tables tb;
  const size_t o_str = tb.add(pl.str), o_grp = tb.add(grp), o_seg = tb.add(small);
  tb.join(large);  // one table: the one-wave form's segments, then the twelve-wave form's
  const size_t o_pool = tb.add(pl.pool), o_ring = tb.add(pl.ringt);
  // (logits and posteriors: K planes of `rows` rows; an every-member call's posteriors once more as the caller's [rows][K])
  const size_t b_pcm = ww_bump::need((size_t)samples, 2), b_rows = ww_bump::need((size_t)rows * F, 4), b_z = ww_bump::need((size_t)rows * K * NO, 4),
               b_post = ww_bump::need((size_t)rows * K, 4);
  if (int rc = ww_ensure(ctx, ctx->dev, tb.bytes() + b_pcm + b_rows + (large.empty() ? 0 : b_z) + (all ? 2 : 1) * b_post + 1024, false)) return rc;
  ww_bump db(ctx->dev.ptr, ctx->dev.cap);
  char *d_tab = db.take<char>(tb.bytes());
  const feed_str *d_str = (const feed_str *)(d_tab + o_str);
  const feed_grp *d_grp = (const feed_grp *)(d_tab + o_grp);
  const wv_feed_seg *d_seg = (const wv_feed_seg *)(d_tab + o_seg);
  const wv_feed_pool *d_pool = (const wv_feed_pool *)(d_tab + o_pool), *d_ringt = (const wv_feed_pool *)(d_tab + o_ring);
  int16_t *d_pcm = db.take<int16_t>((size_t)samples);
  float *d_rows = db.take<float>((size_t)rows * F);
  float *d_z = large.empty() ? nullptr : db.take<float>((size_t)rows * K * NO);
  float *d_post = db.take<float>((size_t)rows * K);
  float *d_post_rows = all ? db.take<float>((size_t)rows * K) : d_post;
  if (int rc = tb.send(ctx, d_tab)) return rc;
  if (st->rates) {  // (the bank's 16 kHz samples land in d_pcm itself)
    std::vector<int64_t> twice;
    if (!byte_offs) {
      twice.resize((size_t)n + 1);
      for (int i = 0; i <= n; ++i) twice[(size_t)i] = 2 * in_offs[i];
      byte_offs = twice.data();
    }
    if (int rc = ww_k_rates_feed(st->rates, ids, n, pcm, byte_offs, sample_offs, d_pcm, mutated)) return rc;
    if (samples == 0) {  // the packets moved the streams' resampling state and completed no 16 kHz sample
      WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
      return WW_OK;
    }
  }
  // ---- from here on the host's mirrors of the streams' state advance
  *mutated = true;
  for (int i = 0; i < n; ++i) {
    const int s = ids[i];
    const int64_t k = sample_offs[i + 1] - sample_offs[i], r = row_offs[i + 1] - row_offs[i];
    st->fill[s] = (int)(st->fill[s] + k - r * hop);
    st->pos[s] = (int)((st->pos[s] + r) % R);
  }
  if (!st->rates) WW_HIP(ctx, hipMemcpyAsync(d_pcm, pcm + sample_offs[0], (size_t)samples * 2, hipMemcpyHostToDevice, ctx->stream));
  feed_fe_args a = {};
  a.pcm = d_pcm; a.str = d_str; a.grp = d_grp; a.rows = d_rows;
  a.ring = st->ring; a.hist = st->hist; a.prev = st->prev;
  a.T = T; a.F = F; a.HR = st->HR;
  a.cv = ww_fe_pcm_of(st->fp);
  a.fb = ww_fe_filt_of(m->filt);
  if (!grp.empty()) {
    ww_launch_scope scope(ctx, "stream_feed_frontend_kernel");
    if (st->fp.precise)
      hipLaunchKernelGGL((stream_feed_frontend_kernel<double>), dim3((unsigned)grp.size()), dim3(FEED_WAVES * 64), feed_fe_lds<double>::bytes, ctx->stream, a);
    else
      hipLaunchKernelGGL((stream_feed_frontend_kernel<float>), dim3((unsigned)grp.size()), dim3(FEED_WAVES * 64), feed_fe_lds<float>::bytes, ctx->stream, a);
    WW_HIP(ctx, hipGetLastError());
  }
  const int pidx = NO == 1 ? 0 : 1;  // posterior element, as a tick's
  if (int rc = ww_k_wave_feed(ctx, m, d_rows, d_seg, (int)small.size(), (int)(small.size() + large.size()), d_pool, (int)pl.pool.size(), d_ringt,
                              (int)pl.ringt.size(), d_z, st->wstate, st->zring, st->zpos, pidx, d_post, st->ref(), all ? K : 0, rows, all ? d_post_rows : nullptr))
    return rc;
  if (rows > 0) WW_HIP(ctx, hipMemcpyAsync(post, d_post_rows, (size_t)rows * K * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (rows > 0 && mel) WW_HIP(ctx, hipMemcpyAsync(mel, d_rows, (size_t)rows * F * 4, hipMemcpyDeviceToHost, ctx->stream));
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return WW_OK;
}

int ww_stream_feed(ww_streams *st, const int32_t *ids, int32_t n, const int16_t *pcm, const int64_t *sample_offs, int64_t cap_rows,
                   int64_t *row_offs, float *post, float *mel) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  if (st->g711()) return ww_fail(st->ctx, WW_EINVAL, "ww_stream_feed: this bank has G.711 streams, its packets are counted in bytes: ww_stream_feed_bytes");
  return st->guarded([&](bool *mutated) { return stream_feed_impl(st, ids, n, pcm, sample_offs, cap_rows, row_offs, post, mel, mutated); });
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// The feed of an every-member causal bank (include/wwhip.h): ww_stream_feed_rows / ww_stream_feed with post [rows][K]
int ww_stream_feed_rows_all(ww_streams *st, const int32_t *ids, int32_t n, const int64_t *sample_offs, int64_t *row_offs) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  return feed_check(st, ids, n, sample_offs, row_offs, "ww_stream_feed_rows_all", nullptr, true);
  WW_GUARD_END(st ? st->ctx : nullptr)
}

int ww_stream_feed_all(ww_streams *st, const int32_t *ids, int32_t n, const int16_t *pcm, const int64_t *sample_offs, int64_t cap_rows,
                       int64_t *row_offs, float *post, float *mel) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  if (st->g711()) return ww_fail(st->ctx, WW_EINVAL, "ww_stream_feed_all: this bank has G.711 streams, its packets are counted in bytes: ww_stream_feed_bytes_all");
  return st->guarded([&](bool *mutated) { return stream_feed_impl(st, ids, n, pcm, sample_offs, cap_rows, row_offs, post, mel, mutated, true); });
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// ww_stream_feed_bytes / _all (include/wwhip.h): the packets' samples are counted per stream format (stream_formats.h: formats_packet)
// - a refusal there, like every other, comes before any state moves -, then the call is ww_stream_feed's: on a bank without G.711
// streams with sample_offs = byte_offs / 2, on a bank with them with the byte offsets beside the sample counts.
static int stream_feed_bytes(ww_streams *st, const int32_t *ids, int32_t n, const void *data, const int64_t *byte_offs, int64_t cap_rows, int64_t *row_offs,
                             float *post, float *mel, bool all) {
  const char *what = all ? "ww_stream_feed_bytes_all" : "ww_stream_feed_bytes";
  std::vector<int64_t> so;
  const bool g711 = st->g711();
  if (n > 0 && ids && byte_offs) {  // (anything else is feed_check's refusal)
    so.assign((size_t)n + 1, g711 ? 0 : byte_offs[0] / 2);
    if (!g711 && (byte_offs[0] & 1)) return ww_fail(st->ctx, WW_EINVAL, "%s: packet 0: an int16 packet starts at byte %lld: an odd offset", what, (long long)byte_offs[0]);
    char why[200];
    for (int i = 0; i < n; ++i) {
      const int s = ids[i];
      const int32_t fmt = g711 && s >= 0 && s < st->S ? ww_k_rates_stream_format(st->rates, s) : WW_SAMPLE_I16;  // (an id out of range: feed_check's refusal)
      int64_t k = 0;
      if (formats_packet(fmt, i, byte_offs[i], byte_offs[i + 1], &k, why, sizeof why)) return ww_fail(st->ctx, WW_EINVAL, "%s: %s", what, why);
      so[(size_t)i + 1] = so[(size_t)i] + k;
    }
  }
  const int64_t *sample_offs = so.empty() ? byte_offs : so.data();
  return st->guarded([&](bool *mutated) {
    return stream_feed_impl(st, ids, n, (const int16_t *)data, sample_offs, cap_rows, row_offs, post, mel, mutated, all, g711 && !so.empty() ? byte_offs : nullptr, what);
  });
}

int ww_stream_feed_bytes(ww_streams *st, const int32_t *ids, int32_t n, const void *data, const int64_t *byte_offs, int64_t cap_rows, int64_t *row_offs,
                         float *post, float *mel) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  return stream_feed_bytes(st, ids, n, data, byte_offs, cap_rows, row_offs, post, mel, false);
  WW_GUARD_END(st ? st->ctx : nullptr)
}

int ww_stream_feed_bytes_all(ww_streams *st, const int32_t *ids, int32_t n, const void *data, const int64_t *byte_offs, int64_t cap_rows, int64_t *row_offs,
                             float *post, float *mel) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  return stream_feed_bytes(st, ids, n, data, byte_offs, cap_rows, row_offs, post, mel, true);
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// ---- host stages of the streaming pipeline for S streams in lock step -------------------------------------------------------
// The reference runs three stage objects per stream and frame (spokestack/pipeline.py:25-28 with demo.py:29-36's stage list):
// VoiceActivityDetector -> WakewordTrigger -> ActivationTimeout, each a few comparisons on the shared SpeechContext.  For S
// streams that is 3 S Python calls per 20 ms tick (round 5: ~220 us of interpreter at 128 streams around a 35 us device tick).
// Here each stage is ONE pass over S streams on plain arrays the host language owns (wwhip/context.py: ContextBank); a stage
// reports the ids whose state changed, so the caller raises activate / deactivate events for those streams only.

// spokestack/vad/webrtc.py:59-77 - run-length hysteresis on the classifier's raw decision; context.is_speech is the state.
int ww_vad_bank_step(int32_t S, const uint8_t *raw, int32_t rise_frames, int32_t fall_frames, uint8_t *run_value,
                     int64_t *run_length, uint8_t *is_speech, int32_t *n_changed) {
  WW_GUARD_BEGIN
  if (S < 0 || (S > 0 && (!raw || !run_value || !run_length || !is_speech))) return WW_EINVAL;
  int changed = 0;
  for (int s = 0; s < S; ++s) {
    const uint8_t r = raw[s] != 0;
    if (r == run_value[s]) {
      ++run_length[s];
    } else {
      run_value[s] = r;
      run_length[s] = 1;
    }
    if (r != (is_speech[s] != 0)) {
      if (r && run_length[s] >= rise_frames) { is_speech[s] = 1; ++changed; }
      if (!r && run_length[s] >= fall_frames) { is_speech[s] = 0; ++changed; }
    }
  }
  if (n_changed) *n_changed = changed;
  return WW_OK;
  WW_GUARD_END(nullptr)
}

// spokestack/wakeword/tflite.py:134-146 (VAD edge, reset on the fall) and :232-239 (running maximum, threshold, activation)
// over the posteriors a tick delivered: the one-slot case of stream_all.h's rule (sa_trigger_update), where it is stated.
int ww_trigger_bank_step(int32_t S, const uint8_t *is_speech, uint8_t *is_active, const float *post, const int32_t *n_post,
                         double threshold, uint8_t *was_speech, float *posterior_max, int32_t *fired_ids, int32_t *n_fired,
                         int32_t *fall_ids, int32_t *n_fall) {
  WW_GUARD_BEGIN
  if (S < 0 || !n_fired || !n_fall || (S > 0 && (!is_speech || !is_active || !post || !n_post || !was_speech || !posterior_max ||
                                                   !fired_ids || !fall_ids)))
    return WW_EINVAL;
  for (int s = 0; s < S; ++s)
    if (n_post[s] < 0 || n_post[s] > 2) return WW_EINVAL;
  sa_trigger_update(S, 1, is_speech, is_active, post, n_post, &threshold, was_speech, posterior_max, fired_ids, nullptr, nullptr, n_fired,
                    fall_ids, n_fall);
  return WW_OK;
  WW_GUARD_END(nullptr)
}

// The trigger stage over K member slots per stream (include/wwhip.h; the rule: stream_all.h, sa_trigger_update)
int ww_trigger_bank_step_all(int32_t S, int32_t K, const uint8_t *is_speech, uint8_t *is_active, const float *post, const int32_t *n_post,
                             const double *thresholds, uint8_t *was_speech, float *posterior_max, int32_t *fired_ids, int32_t *fired_slot,
                             uint64_t *fired_mask, int32_t *n_fired, int32_t *fall_ids, int32_t *n_fall) {
  WW_GUARD_BEGIN
  if (sa_check_trigger(S, K, is_speech, is_active, post, n_post, thresholds, was_speech, posterior_max, fired_ids, fired_slot, fired_mask, n_fired,
                       fall_ids, n_fall, nullptr, 0))
    return WW_EINVAL;
  sa_trigger_update(S, K, is_speech, is_active, post, n_post, thresholds, was_speech, posterior_max, fired_ids, fired_slot, fired_mask, n_fired,
                    fall_ids, n_fall);
  return WW_OK;
  WW_GUARD_END(nullptr)
}

// spokestack/activation_timeout.py:25-38.  min_frames / max_frames are the reference's quotients (min_active / frame_width), kept
// as doubles: the comparisons are int > float there.
int ww_timeout_bank_step(int32_t S, const uint8_t *is_speech, uint8_t *is_active, uint8_t *was_speech, int32_t *active_frames,
                         double min_frames, double max_frames, int32_t *deact_ids, int32_t *n_deact) {
  WW_GUARD_BEGIN
  if (S < 0 || !n_deact || (S > 0 && (!is_speech || !is_active || !was_speech || !active_frames || !deact_ids))) return WW_EINVAL;
  int nd = 0;
  for (int s = 0; s < S; ++s) {
    const uint8_t sp = is_speech[s] != 0;
    const bool fell = was_speech[s] && !sp;
    was_speech[s] = sp;
    if (!is_active[s]) continue;
    const int len = ++active_frames[s];
    if ((double)len > min_frames && (fell || (double)len > max_frames)) {
      active_frames[s] = 0;
      is_active[s] = 0;
      deact_ids[nd++] = s;
    }
  }
  *n_deact = nd;
  return WW_OK;
  WW_GUARD_END(nullptr)
}

}  // extern "C"

// WakewordTrigger.__call__ for S streams as ONE call: the tick (ww_stream_step with bit 0 = is_speech, bit 1 = is_active as they
// stand BEFORE the tick), then ww_trigger_bank_step over its posteriors, then WakewordTrigger.reset for the streams whose VAD bit
// fell (tflite.py:143-146).  is_active is updated in place.
// Every: the stage of an every-member bank (K slots per stream, the tick ww_stream_step_all); else K = 1 - one threshold, the slot and
// mask lists not asked for (nullptr, as sa_trigger_update permits) -, known where the rule's loops are compiled.
template <bool Every>
static int stream_step_trigger(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, uint8_t *is_active, const double *thresholds,
                               uint8_t *was_speech, float *posterior_max, float *post, int32_t *n_post, int32_t *fired_ids,
                               int32_t *fired_slot, uint64_t *fired_mask, int32_t *n_fired, int32_t *fall_ids, int32_t *n_fall) {
  if (!is_speech || !is_active || !thresholds || !was_speech || !posterior_max || !fired_ids || !n_fired || !fall_ids || !n_fall ||
      (Every && (!fired_slot || !fired_mask)))
    return ww_fail(st->ctx, WW_EINVAL, "NULL argument");
  if (int rc = st->check_call(Every ? "ww_stream_step_trigger_all" : "ww_stream_step_trigger", Every)) return rc;
  *n_fired = *n_fall = 0;
  st->stage_flags.resize((size_t)st->S);
  for (int s = 0; s < st->S; ++s) st->stage_flags[s] = (uint8_t)((is_speech[s] != 0) | ((is_active[s] != 0) << 1));
  int rc = stream_step_entry(st, frames, st->stage_flags.data(), post, n_post, Every ? "ww_stream_step_all" : "ww_stream_step", Every);
  if (rc) return rc;
  sa_trigger_update(st->S, Every ? st->K : 1, is_speech, is_active, post, n_post, thresholds, was_speech, posterior_max, fired_ids, fired_slot,
                    fired_mask, n_fired, fall_ids, n_fall);
  if (*n_fall) rc = ww_stream_reset(st, fall_ids, *n_fall);
  return rc;
}

extern "C" {

int ww_stream_step_trigger(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, uint8_t *is_active, double threshold,
                           uint8_t *was_speech, float *posterior_max, float *post, int32_t *n_post, int32_t *fired_ids,
                           int32_t *n_fired, int32_t *fall_ids, int32_t *n_fall) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  return stream_step_trigger<false>(st, frames, is_speech, is_active, &threshold, was_speech, posterior_max, post, n_post, fired_ids, nullptr, nullptr,
                                    n_fired, fall_ids, n_fall);
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// The wake-word stage of an every-member bank as ONE call (include/wwhip.h): the K-slot rule, and which slot it was
int ww_stream_step_trigger_all(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, uint8_t *is_active, const double *thresholds,
                               uint8_t *was_speech, float *posterior_max, float *post, int32_t *n_post, int32_t *fired_ids,
                               int32_t *fired_slot, uint64_t *fired_mask, int32_t *n_fired, int32_t *fall_ids, int32_t *n_fall) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  return stream_step_trigger<true>(st, frames, is_speech, is_active, thresholds, was_speech, posterior_max, post, n_post, fired_ids, fired_slot,
                                   fired_mask, n_fired, fall_ids, n_fall);
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// The three stages of a tick in one call (include/wwhip.h): exactly the three entry points above, in stage order.
int ww_pipeline_bank_step(ww_streams *st, const int16_t *frames, ww_pipeline_state *ps) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  if (!ps) return ww_fail(st->ctx, WW_EINVAL, "NULL state block");
  if (int rc = st->check_call("ww_pipeline_bank_step", false)) return rc;  // (before the VAD stage moves)
  ps->n_vad_changed = ps->n_fired = ps->n_fall = ps->n_deact = 0;
  int rc = ww_vad_bank_step(st->S, ps->raw, ps->rise_frames, ps->fall_frames, ps->run_value, ps->run_length, ps->is_speech, &ps->n_vad_changed);
  if (rc) return ww_fail(st->ctx, rc, "ww_pipeline_bank_step: the VAD stage's arrays");
  rc = ww_stream_step_trigger(st, frames, ps->is_speech, ps->is_active, ps->threshold, ps->wake_was_speech, ps->posterior_max, ps->post,
                              ps->n_post, ps->fired_ids, &ps->n_fired, ps->fall_ids, &ps->n_fall);
  if (rc) return rc;
  rc = ww_timeout_bank_step(st->S, ps->is_speech, ps->is_active, ps->timeout_was_speech, ps->active_frames, ps->min_frames, ps->max_frames,
                            ps->deact_ids, &ps->n_deact);
  if (rc) return ww_fail(st->ctx, rc, "ww_pipeline_bank_step: the timeout stage's arrays");
  return WW_OK;
  WW_GUARD_END(st ? st->ctx : nullptr)
}

int ww_stream_timeline(ww_streams *st, double *mean_ns, int64_t *ticks, int32_t reset) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  if (ticks) *ticks = st->tl_ticks;
  if (mean_ns)
    for (int i = 0; i < WW_STREAM_TL_PHASES; ++i) mean_ns[i] = st->tl_ticks ? (double)st->tl_ns[i] / (double)st->tl_ticks : 0.0;
  if (reset) {
    memset(st->tl_ns, 0, sizeof(st->tl_ns));
    st->tl_ticks = 0;
  }
  return WW_OK;
  WW_GUARD_END(st ? st->ctx : nullptr)
}

}  // extern "C"

// ---- a CTC stream bank (include/wwhip.h; stream_ctc.h) ----------------------------------------------------------------------------------
// ww_stream_step_ctc's refusals - all before any state moves -, then the one tick
static int stream_step_ctc_entry(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, int32_t max_labels, int32_t *labels,
                                 int32_t *lengths, float *steps, int32_t *n_post, const char *call, float *scores = nullptr,
                                 float *align_value = nullptr, int8_t *align_span = nullptr, const st_ctc_out *beam = nullptr) {
  ww_ctx *ctx = st->ctx;
  if (int rc = st->check_call(call, false, true)) return rc;
  if (int rc = st->check_sound()) return rc;
  if (max_labels < 1 || max_labels > WW_STREAM_CTC_MAX_LABELS)
    return ww_fail(ctx, WW_EINVAL, "%s: max_labels %d: a streamed window carries 1..%d labels", call, (int)max_labels, WW_STREAM_CTC_MAX_LABELS);
  if (!labels || !lengths) return ww_fail(ctx, WW_EINVAL, "%s: NULL argument", call);
  if (steps && !st->ctc_steps) return ww_fail(ctx, WW_EINVAL, "%s: posteriors are returned by a bank created with WW_STREAM_CTC_STEPS", call);
  st_ctc_out co = {max_labels, labels, lengths, steps, scores, align_value, align_span};
  if (beam) {
    co.beam_width = beam->beam_width; co.top_paths = beam->top_paths; co.beam_max_labels = beam->beam_max_labels;
    co.beam_labels = beam->beam_labels; co.beam_lengths = beam->beam_lengths; co.beam_probs = beam->beam_probs;
  }
  return stream_step_entry(st, frames, is_speech, nullptr, n_post, call, false, &co);
}

extern "C" {

int ww_stream_create_ctc(ww_ctx *ctx, const ww_model *model, int32_t S, const ww_frontend_params *fp, uint32_t flags, ww_streams **out) {
  WW_GUARD_BEGIN
  if (!ctx || !model || !fp || !out) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  *out = nullptr;
  if (int rc = ww_crnn_ctc_check(ctx, model, "ww_stream_create_ctc")) return rc;
  if (flags & WW_STREAM_CAUSAL) return ww_fail(ctx, WW_EINVAL, "ww_stream_create_ctc: WW_STREAM_CAUSAL is the fp32 Wavenet's sequence form, not a CRNN's");
  if (flags & ~(uint32_t)(WW_STREAM_FULL_RECOMPUTE | WW_STREAM_TWO_LAUNCH | WW_STREAM_SYNC_WAIT | WW_STREAM_CTC_STEPS))
    return ww_fail(ctx, WW_EINVAL, "ww_stream_create_ctc: unknown stream flags 0x%x", flags);
  return stream_create_impl(ctx, model, nullptr, nullptr, S, fp, flags, out, 0, true);
  WW_GUARD_END(ctx)
}

int ww_stream_step_ctc(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, int32_t max_labels, int32_t *labels, int32_t *lengths,
                       float *steps, int32_t *n_post) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  return stream_step_ctc_entry(st, frames, is_speech, max_labels, labels, lengths, steps, n_post, "ww_stream_step_ctc");
  WW_GUARD_END(st ? st->ctx : nullptr)
}

int ww_stream_ctc_set_targets(ww_streams *st, const int32_t *targets, const int32_t *target_lens, int32_t K, int32_t mode) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  const char *call = "ww_stream_ctc_set_targets";
  ww_ctx *ctx = st->ctx;
  if (int rc = st->check_call(call, false, true)) return rc;
  if (!st->ctc_steps) return ww_fail(ctx, WW_EINVAL, "%s: the score is computed from a tick's posteriors: the bank must be created with WW_STREAM_CTC_STEPS", call);
  char why[200];
  if (!ww_ctc_score_args_ok(WW_SC_STEPS, st->NO, targets, target_lens, K, mode, why, sizeof why)) return ww_fail(ctx, WW_EINVAL, "%s: %s", call, why);
  if (!st->h_score) {
    WW_ON_DEVICE(ctx, dev_scope);
    if (hipHostMalloc((void **)&st->h_score, (size_t)2 * st->S * WW_CTC_SCORE_MAX_TARGETS * 4) != hipSuccess) {
      st->h_score = nullptr;
      return ww_fail(ctx, WW_ENOMEM, "%s: cannot allocate the score block of %d streams", call, st->S);
    }
    if (hipHostGetDevicePointer((void **)&st->h_score_dev, st->h_score, 0) != hipSuccess) return ww_fail(ctx, WW_EHIP, "%s: the score block is not visible to the device", call);
  }
  ww_ctc_score_targets &tg = st->score_tg;
  memset(&tg, 0, sizeof tg);
  tg.K = K;
  tg.mode = mode;
  for (int k = 0; k < K; ++k) {
    tg.len[k] = (int8_t)target_lens[k];
    for (int u = 0; u < target_lens[k]; ++u) tg.c[k][u] = (int8_t)targets[k * WW_CTC_SCORE_MAX_TARGET + u];
  }
  st->score_set = true;
  return WW_OK;
  WW_GUARD_END(st ? st->ctx : nullptr)
}

int ww_stream_step_ctc_score(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, int32_t max_labels, int32_t *labels,
                             int32_t *lengths, float *steps, float *scores, int32_t *n_post) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  const char *call = "ww_stream_step_ctc_score";
  if (int rc = st->check_call(call, false, true)) return rc;
  if (!st->score_set) return ww_fail(st->ctx, WW_EINVAL, "%s: the bank has no targets (ww_stream_ctc_set_targets)", call);
  if (!scores) return ww_fail(st->ctx, WW_EINVAL, "%s: NULL argument", call);
  return stream_step_ctc_entry(st, frames, is_speech, max_labels, labels, lengths, steps, n_post, call, scores);
  WW_GUARD_END(st ? st->ctx : nullptr)
}

int ww_stream_step_ctc_align(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, int32_t max_labels, int32_t *labels,
                             int32_t *lengths, float *steps, float *scores, float *align_value, int8_t *align_span, int32_t *n_post) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  const char *call = "ww_stream_step_ctc_align";
  ww_ctx *ctx = st->ctx;
  if (int rc = st->check_call(call, false, true)) return rc;
  if (!st->ctc_steps) return ww_fail(ctx, WW_EINVAL, "%s: the alignment is computed from a tick's posteriors: the bank must be created with WW_STREAM_CTC_STEPS", call);
  if (!st->score_set) return ww_fail(ctx, WW_EINVAL, "%s: the bank has no targets (ww_stream_ctc_set_targets)", call);
  if (!scores || !align_value || !align_span) return ww_fail(ctx, WW_EINVAL, "%s: NULL argument", call);
  if (!st->h_align) {
    WW_ON_DEVICE(ctx, dev_scope);
    const size_t slots = (size_t)2 * st->S * WW_CTC_SCORE_MAX_TARGETS;
    if (hipHostMalloc((void **)&st->h_align, slots * (4 + 2 * WW_CTC_SCORE_MAX_TARGET)) != hipSuccess) {
      st->h_align = nullptr;
      return ww_fail(ctx, WW_ENOMEM, "%s: cannot allocate the alignment block of %d streams", call, st->S);
    }
    if (hipHostGetDevicePointer((void **)&st->h_align_dev, st->h_align, 0) != hipSuccess) {
      hipHostFree(st->h_align);
      st->h_align = nullptr;
      return ww_fail(ctx, WW_EHIP, "%s: the alignment block is not visible to the device", call);
    }
  }
  return stream_step_ctc_entry(st, frames, is_speech, max_labels, labels, lengths, steps, n_post, call, scores, align_value, align_span);
  WW_GUARD_END(st ? st->ctx : nullptr)
}

int ww_stream_step_ctc_beam(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, int32_t max_labels, int32_t *labels,
                            int32_t *lengths, float *steps, int32_t beam_width, int32_t top_paths, int32_t beam_max_labels, int32_t *beam_labels,
                            int32_t *beam_lengths, float *beam_probs, int32_t *n_post) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  const char *call = "ww_stream_step_ctc_beam";
  ww_ctx *ctx = st->ctx;
  if (int rc = st->check_call(call, false, true)) return rc;
  if (!st->ctc_steps) return ww_fail(ctx, WW_EINVAL, "%s: the beam search reads a tick's posteriors: the bank must be created with WW_STREAM_CTC_STEPS", call);
  char why[200];
  if (!ww_ctc_beam_args_ok(WW_SC_STEPS, st->NO, beam_width, top_paths, beam_max_labels, why, sizeof why)) return ww_fail(ctx, WW_EINVAL, "%s: %s", call, why);
  if (!beam_labels || !beam_lengths || !beam_probs) return ww_fail(ctx, WW_EINVAL, "%s: beam_labels / beam_lengths / beam_probs are NULL", call);
  if (!st->h_beam) {
    WW_ON_DEVICE(ctx, dev_scope);
    if (hipHostMalloc((void **)&st->h_beam, st->beam_words() * 4) != hipSuccess) {
      st->h_beam = nullptr;
      return ww_fail(ctx, WW_ENOMEM, "%s: cannot allocate the beam block of %d streams", call, st->S);
    }
    if (hipHostGetDevicePointer((void **)&st->h_beam_dev, st->h_beam, 0) != hipSuccess) {
      hipHostFree(st->h_beam);
      st->h_beam = nullptr;
      return ww_fail(ctx, WW_EHIP, "%s: the beam block is not visible to the device", call);
    }
  }
  st_ctc_out beam;
  beam.beam_width = beam_width; beam.top_paths = top_paths; beam.beam_max_labels = beam_max_labels;
  beam.beam_labels = beam_labels; beam.beam_lengths = beam_lengths; beam.beam_probs = beam_probs;
  return stream_step_ctc_entry(st, frames, is_speech, max_labels, labels, lengths, steps, n_post, call, nullptr, nullptr, nullptr, &beam);
  WW_GUARD_END(st ? st->ctx : nullptr)
}

// ww_ctc_trigger_bank_step with the score rule (stream_ctc.h: sc_score_trigger_update, where the rule is stated)
int ww_ctc_score_trigger_bank_step(int32_t S, int32_t K, const uint8_t *is_speech, uint8_t *is_active, const float *scores, const int32_t *n_post,
                                   const double *thresholds, uint8_t *was_speech, int32_t *fired_ids, int32_t *fired_slot, int32_t *n_fired,
                                   int32_t *fall_ids, int32_t *n_fall) {
  WW_GUARD_BEGIN
  if (sc_check_score_trigger(S, K, is_speech, is_active, scores, n_post, thresholds, was_speech, fired_ids, fired_slot, n_fired, fall_ids, n_fall))
    return WW_EINVAL;
  sc_score_trigger_update(S, K, is_speech, is_active, scores, n_post, thresholds, was_speech, fired_ids, fired_slot, n_fired, fall_ids, n_fall);
  return WW_OK;
  WW_GUARD_END(nullptr)
}

// ww_trigger_bank_step with the label rule in place of the threshold (stream_ctc.h: sc_trigger_update, where the rule is stated)
int ww_ctc_trigger_bank_step(int32_t S, const uint8_t *is_speech, uint8_t *is_active, const int32_t *labels, const int32_t *lengths,
                             const int32_t *n_post, int32_t max_labels, const int32_t *target, int32_t n_target, uint8_t *was_speech,
                             int32_t *fired_ids, int32_t *n_fired, int32_t *fall_ids, int32_t *n_fall) {
  WW_GUARD_BEGIN
  if (sc_check_trigger(S, is_speech, is_active, labels, lengths, n_post, max_labels, target, n_target, was_speech, fired_ids, n_fired, fall_ids, n_fall))
    return WW_EINVAL;
  sc_trigger_update(S, is_speech, is_active, labels, lengths, n_post, max_labels, target, n_target, was_speech, fired_ids, n_fired, fall_ids, n_fall);
  return WW_OK;
  WW_GUARD_END(nullptr)
}

// ww_stream_step_trigger for a CTC bank: the tick (bit 0 = is_speech, bit 1 = is_active as they stand BEFORE the tick), the label
// rule over its decodes, then the reset of the streams whose VAD bit fell.  is_active is updated in place.
int ww_stream_step_ctc_trigger(ww_streams *st, const int16_t *frames, const uint8_t *is_speech, uint8_t *is_active, int32_t max_labels,
                               const int32_t *target, int32_t n_target, uint8_t *was_speech, int32_t *labels, int32_t *lengths, float *steps,
                               int32_t *n_post, int32_t *fired_ids, int32_t *n_fired, int32_t *fall_ids, int32_t *n_fall) {
  WW_GUARD_BEGIN
  if (!st) return WW_EINVAL;
  const char *call = "ww_stream_step_ctc_trigger";
  if (int rc = st->check_call(call, false, true)) return rc;
  if (!is_speech || !is_active || !target || !was_speech || !n_post || !fired_ids || !n_fired || !fall_ids || !n_fall)
    return ww_fail(st->ctx, WW_EINVAL, "%s: NULL argument", call);
  if (max_labels < 1 || max_labels > WW_STREAM_CTC_MAX_LABELS || n_target < 1 || n_target > max_labels)
    return ww_fail(st->ctx, WW_EINVAL, "%s: max_labels %d (1..%d), a target of %d labels (1..max_labels)", call, (int)max_labels,
                   WW_STREAM_CTC_MAX_LABELS, (int)n_target);
  *n_fired = *n_fall = 0;
  st->stage_flags.resize((size_t)st->S);
  for (int s = 0; s < st->S; ++s) st->stage_flags[s] = (uint8_t)((is_speech[s] != 0) | ((is_active[s] != 0) << 1));
  int rc = stream_step_ctc_entry(st, frames, st->stage_flags.data(), max_labels, labels, lengths, steps, n_post, call);
  if (rc) return rc;
  sc_trigger_update(st->S, is_speech, is_active, labels, lengths, n_post, max_labels, target, n_target, was_speech, fired_ids, n_fired, fall_ids, n_fall);
  if (*n_fall) rc = ww_stream_reset(st, fall_ids, *n_fall);
  return rc;
  WW_GUARD_END(st ? st->ctx : nullptr)
}

}  // extern "C"
