// The per-stream front end of a streaming tick (spokestack/wakeword/tflite.py:148-191), once, for the four kernels that run it:
//   stream_frontend_kernel<R>       streams.hip   two-launch tick, causal tick
//   stream_feed_frontend_kernel<R>  streams.hip   ww_stream_feed
//   crnn_stream_kernel<FE = 1, 2>   crnn.hip      one-launch CRNN tick
//   wavenet_kernel<..., TICK>       wavenet.hip   one-launch Wavenet tick
// How a stream's samples become mel rows and where the rows go is decided here: int16 -> float, clip and pre-emphasis against the
// carried sample; Hann, rFFT, |.|, mel of one new frame by one wave (fft_device.h); the row's two slots in the mirrored ring; the
// one-launch tick's control words and its mel-side LDS.  The kernels call the same functions on the same values, so the same
// samples give the same bits in every form by construction.  What the kernels keep to themselves is their load prologue (what is
// requested before the branch on the control words, and in which order): those orders were measured per kernel.
#pragma once
#include "common.h"
#include "fft_device.h"

#define WW_ST_RING 832  // a stream's sample ring: 511 pending samples + the 320 of a tick, rounded up
#define FE_MAG_LD 260   // floats between two waves' magnitudes (257 used)

// ---- what the kernels are told ---------------------------------------------------------------------------------------------------
// the model's filterbank and the transform's constants (ww_filter_dev)
struct ww_fe_filt {
  const int *start;
  const float *wpad, *bias;
  int n_mel;
  float floor_v, log_off, scale;
  const double *hann, *tw256, *tw512;
};
static inline ww_fe_filt ww_fe_filt_of(const ww_filter_dev &f) {
  return {f.start, f.wpad, f.bias, f.n_mel, f.floor_v, f.log_off, f.scale, f.hann, f.tw256, f.tw512};
}
// int16 -> sample (ww_frontend_params)
struct ww_fe_pcm {
  float divisor;
  int clip;
  float preemph;
};
static inline ww_fe_pcm ww_fe_pcm_of(const ww_frontend_params &fp) { return {fp.pcm_divisor, fp.clip, fp.pre_emphasis}; }

// The streaming front end's side of a ONE-launch tick (crnn_stream_kernel<FE != 0>, wavenet_kernel<..., TICK>).  Workgroup 2 s + k is
// window k of stream s's tick; it reads the stream's control words and samples over the bus itself.
struct ww_tick_fe {
  const int16_t *frames;  // page-locked host memory [S][WW_CHUNK]
  const int32_t *ctl;     // page-locked host memory [S][4]: fill, n_frames, flags (1 speech, 2 active, 4 state parity), pos | rowq << 16
  float *ring;            // [2][S][WW_ST_RING]: a stream's sample ring, ping-pong by its state parity (read [par], written [par ^ 1])
  float *prev;            // [2][S] pre-emphasis carry, likewise
  float *hist;            // [S][HR][F] mirrored mel rings (the model's `mel`)
  int S, HR;
  ww_fe_pcm cv;
  int hop;
};

// frames that `tot` buffered samples complete (tflite.py:163-168: one whenever 512 are buffered, then the oldest `hop` are dropped)
static inline int64_t ww_fe_frames(int64_t tot, int hop) { return tot >= WW_FFT_WINDOW ? (tot - WW_FFT_WINDOW) / hop + 1 : 0; }

#ifdef __HIPCC__
// ---- sample conversion -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fe_norm(int16_t v, const ww_fe_pcm &c) {
  float x = __fdiv_rn((float)v, c.divisor);
  if (c.clip) x = fminf(fmaxf(x, -1.0f), 1.0f);
  return x;
}
// sample i of a packet xs (LDS or global int16), `carry` = the un-emphasised sample in front of it.  (A branch, not a select: a
// select would read xs[-1].)
template <typename SRC, typename I>
__device__ __forceinline__ float fe_sample(SRC xs, I i, float carry, const ww_fe_pcm &c) {
  const float v = fe_norm(xs[i], c);
  float p;
  if (i == 0) {
    p = carry;
  } else {
    p = fe_norm(xs[i - 1], c);
  }
  return (c.preemph != 0.0f) ? ww_preemph_rn(v, c.preemph, p) : v;
}

// ---- one new frame by one wave: x = its 512 samples in LDS, `slot` = the wave's exchange buffer and magnitudes; returns band `lane`
template <typename R>
__device__ __forceinline__ float fe_frame_mel(const float *x, const fft_consts<R> &fc, cplx<R> *buf, float *mag, int slot, const float *wl,
                                              int mel_st, float mel_bias, const ww_fe_filt &fb, int lane) {
  auto x2 = [&](int n) -> float2 { return make_float2(x[2 * n], x[2 * n + 1]); };
  float *mg = mag + slot * FE_MAG_LD;
  frame_fft_mag<R>(x2, fc, buf + slot * FFT_LD, mg, lane);
  return mel_band(mg, wl, mel_st, mel_bias, fb.floor_v, fb.log_off, fb.scale, lane);
}

// ---- mirrored ring of `slots` = T + 1 rows (streams.hip) that starts at row `row0` of hist: row p (< 2 slots) goes to p % slots
// and p % slots + slots
__device__ __forceinline__ void fe_ring_store(float *hist, size_t row0, int p, int slots, int F, int lane, float mv) {
  p = p >= slots ? p - slots : p;
  float *h = hist + (row0 + p) * F + lane;
  h[0] = mv;
  h[(size_t)slots * F] = mv;
}

// ---- the one-launch tick: what workgroup 2 s + k is (uniform over it) ----------------------------------------------------------------
// A bank that runs K member slots on every stream (stream_all.h): workgroup 2 v + k, v = s K + slot, is window k of member slot `slot`
// on stream s.  The 2 K workgroups of a stream read the same control words; the stream's state is written by slot 0's writer alone,
// and a slot other than 0 that has no window has nothing to do at all.
struct fe_tick_ctl {
  int fill, nf, pos, rowq;  // rowq: the CRNN's (rows since the reset, mod its cache ring)
  int par, np;
  bool idle;                // an active stream is not sampled at all (tflite.py:139-140) | the tick has no second window
  bool window, writer;      // this workgroup evaluates a window | writes the stream's state (the tick's newest window, or none at all; slot 0)
  int nfk;                  // window k ends at new frame k: it needs frames 0..k
  int b;                    // the T rows that end at new row k are the contiguous block from slot (pos + k + 2) % slots
};
__device__ __forceinline__ fe_tick_ctl fe_tick_decode(int4 cw, int k, int slots, int slot = 0) {
  fe_tick_ctl c;
  c.fill = cw.x; c.nf = cw.y; c.pos = cw.w & 0xffff; c.rowq = cw.w >> 16;
  const int flags = cw.z;
  c.par = (flags >> 2) & 1;
  c.np = (flags & 1) ? c.nf : 0;  // frames are analysed only while the VAD says speech (tflite.py:166)
  c.idle = (flags & 2) || k >= (c.np > 1 || slot != 0 ? c.np : 1);
  c.window = k < c.np; c.writer = k + 1 >= c.np && slot == 0;
  c.nfk = c.window ? k + 1 : 0;
  c.b = c.pos + k + 2;
  c.b = c.b >= slots ? c.b - slots : c.b;
  return c;
}

// ---- the one-launch tick's mel-side LDS, in floats from a 16-byte aligned base inside a region its kernel has free at that point
#define FE_TL_X 0                                   // [WW_ST_RING] ring | the tick's new samples
#define FE_TL_XS (FE_TL_X + WW_ST_RING)             // [WW_CHUNK] int16: the raw samples
#define FE_TL_WL (FE_TL_XS + WW_CHUNK / 2)          // [3072] the mel weights [WW_MEL_TAPS][64], padded to whole store rounds of 768 x 16 bytes
#define FE_TL_MAG (FE_TL_WL + 3072)                 // [2][FE_MAG_LD] magnitudes of the (at most) two new frames
#define FE_TL_BUF (FE_TL_MAG + 2 * FE_MAG_LD + 8)   // [2][FFT_LD] complex: the transforms' exchange buffers
#define FE_TL_FLOATS (FE_TL_BUF + 2 * FFT_LD * 4)
static_assert(FE_TL_WL % 4 == 0 && FE_TL_BUF % 4 == 0 && WW_MEL_TAPS * 64 <= 3072 && WW_CHUNK * 2 == 40 * 16,
              "tick front end: 16-byte aligned weights and exchange buffers, the weights' store rounds, a tick's 40 sixteen-byte pieces");
template <typename R>
struct fe_tick_lds {
  float *x, *wl, *mag;
  short *xs;
  cplx<R> *buf;
};
// (an initialiser list in the kernel, not a function: behind a function's parameter wavenet_kernel's constant LDS addresses folded
// into its transform's stores differently - three more address instructions)
#define FE_TICK_LDS(R, base) \
  fe_tick_lds<R> { (base) + FE_TL_X, (base) + FE_TL_WL, (base) + FE_TL_MAG, (short *)((base) + FE_TL_XS), (cplx<R> *)((base) + FE_TL_BUF) }
#endif
