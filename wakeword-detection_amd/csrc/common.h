// Internal declarations shared by the libwwhip.so translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/wwhip.h"
#include "events_plan.h"
#include "launch_plan.h"
#include "model_layout.h"
#include "stream_rate.h"
#include "stream_rates.h"
#include "stream_formats.h"

#define WW_WAVE 64

struct ww_prof_entry {
  int calls = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double total_ms = 0.0;
};

// Growable device / pinned-host arenas: ensure() is called by the entry points before they start enqueueing.
struct ww_arena {
  void *ptr = nullptr;
  size_t cap = 0;
};

struct ww_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  char err[512] = {0};
  ww_arena dev;     // device workspace
  ww_arena pinned;  // pinned host staging
  bool profiling = false;
  std::map<std::string, ww_prof_entry> prof;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  // sample/frame offset tables of the equal-length clip batches seen so far (tiny, built once)
  struct clip_offs_t {
    int n_clips = 0, samples = 0, hop = 0;
    int64_t *d_so = nullptr, *d_fo = nullptr;
  };
  std::vector<clip_offs_t> clip_offs;
  // launch tables on their way to the device (ww_tables::send, the only code that touches these): two page-locked slots used
  // alternately, each free again once the event behind its copy has passed
  ww_arena desc_pin[2];
  hipEvent_t desc_ev[2] = {nullptr, nullptr};
  bool desc_busy[2] = {false, false};
  unsigned desc_k = 0;
};

// (ww_filter_dev, ww_crnn_dev, ww_wave_dev - model_layout.h's scalar geometry plus the pointers into a model's device block - are
// model_layout.h's too: model_set.h translates them on the host)
struct ww_model {
  ww_ctx *ctx = nullptr;
  int kind = 0;
  ww_model_info info = {};
  ww_filter_dev filt;
  ww_crnn_dev crnn;
  ww_wave_dev wave;
  int precision = 0;  // WW_PRECISION_*
  int opt_split_at = 1024;  // WW_OPT_CRNN_SPLIT_AT
  int opt_slide_min = 64;   // WW_OPT_CRNN_SLIDE_MIN
  int opt_tail_mfma = 1;    // WW_OPT_CRNN_TAIL_MFMA
  int opt_wave_rowmajor = 0;  // WW_OPT_WAVENET_ROWMAJOR
  int opt_wave_seq_segment = 0;  // WW_OPT_WAVE_SEQ_SEGMENT (0 = the library's choice)
  void *block = nullptr;  // the one device allocation behind every pointer of filt, crnn and wave
  size_t block_bytes = 0;           // its size: a function of the geometry alone (model_pack.h)
  std::vector<uint8_t> filt_image;  // the filter's arrays as the packer made them (model_set.h: ww_set_filter_image): what two
                                    // members of a set must share
};

// K models of one geometry behind one launch (include/wwhip.h: ww_model_set_create; the host half is model_set.h).  The members'
// blocks lie at block + k * stride; `view` is member 0 with every pointer translated into that allocation - what the launchers
// build their kernel arguments from - and owns nothing.
struct ww_model_set {
  ww_ctx *ctx = nullptr;
  int n = 0;
  size_t stride = 0;
  void *block = nullptr;
  ww_model view;
};

// A SET kernel's extra argument (crnn_fused_kernel, crnn_stream_kernel, wavenet_kernel, wavenet_seq_kernel with SET = true): the
// workgroup's member is ids[i], i by the launch form - a batch: the workgroup's window; a one-launch tick: its stream; a
// table-driven tick: the stream in its window's aux word (aux != nullptr: a Wavenet window bank's kernel has no other use for that
// table); a feed: its segment's stream - and every weight pointer of the kernel's arguments moves on by member * stride bytes.
// The SET = false instantiations take the same (empty) argument and never look at it.
// The sliding form's kernels (crnn_rows_kernel, gru_tail_kernel, gru_tail16_kernel with SET = true) index ids by blockIdx.y - the
// call's member slot, a grid dimension - and read the sizes of their member-major planes from aux (crnn.hip: WW_SLIDE_AUX_*).
// The Wavenet's whole-sequence form (wavenet_seq_kernel<12, false, false, true>) indexes ids by blockIdx.y as well - the slot is the
// output plane - unless aux is given: then aux[blockIdx.x] is the segment's sequence and ids holds one member per sequence.
struct ww_set_ref {
  const int32_t *ids = nullptr;
  const int32_t *aux = nullptr;
  long long stride = 0;
};

int ww_fail(ww_ctx *ctx, int code, const char *fmt, ...);
int ww_ensure(ww_ctx *ctx, ww_arena &a, size_t bytes, bool pinned);

// No exception crosses the C ABI (every entry point returns a status, never throws): the body of every exported
// function sits between WW_GUARD_BEGIN and WW_GUARD_END(ctx) - std::bad_alloc from a container or `new` becomes WW_ENOMEM,
// anything else WW_EINTERNAL, with the text where ww_last_error finds it (ctx may be nullptr: the thread's text).  The few
// exported functions that only read a field or return a constant carry WW_NOTHROW instead (tests/test_cabi_and_dist.py
// checks that every definition has one or the other).
#define WW_GUARD_BEGIN try {
#define WW_GUARD_END(ctx_)                                                                                  \
  }                                                                                                         \
  catch (const std::bad_alloc &) { return ww_fail((ctx_), WW_ENOMEM, "%s: out of host memory", __func__); } \
  catch (const std::exception &e_) { return ww_fail((ctx_), WW_EINTERNAL, "%s: %s", __func__, e_.what()); } \
  catch (...) { return ww_fail((ctx_), WW_EINTERNAL, "%s: unknown exception", __func__); }
// An object a create function has allocated and not yet handed out: destroyed if the function leaves early (an error
// return, or an exception on its way to WW_GUARD_END).
template <typename T, int (*Destroy)(T *)>
struct ww_scoped {
  T *p;
  explicit ww_scoped(T *q) : p(q) {}
  ww_scoped(const ww_scoped &) = delete;
  ~ww_scoped() {
    if (p) Destroy(p);
  }
  T *release() {
    T *r = p;
    p = nullptr;
    return r;
  }
};
#define WW_NOTHROW /* marker: the body allocates nothing and calls nothing that can throw */

#define WW_HIP(ctx, expr)                                                                       \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return ww_fail((ctx), WW_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// The device-pointer entry points enqueue on the context's stream without touching the caller's
// current device (the caller may be a framework that tracks it): switch only if needed, and restore.
struct ww_device_scope {
  int prev = -1;
  bool changed = false;
  hipError_t err = hipSuccess;  // why the switch to `dev` failed; entry points check ok() before they allocate or launch
  explicit ww_device_scope(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) {
      err = hipSetDevice(dev);
      changed = err == hipSuccess;
    }
  }
  bool ok() const { return err == hipSuccess; }
  ~ww_device_scope() {
    if (changed) (void)hipSetDevice(prev);
  }
};
// Declares the scope and leaves the entry point with WW_EHIP if the context's device could not be made current.
#define WW_ON_DEVICE(ctx_, name_)                                                                                   \
  ww_device_scope name_((ctx_)->device);                                                                            \
  if (!name_.ok())                                                                                                  \
    return ww_fail((ctx_), WW_EHIP, "cannot switch to device %d: %s", (ctx_)->device, hipGetErrorString(name_.err))

// Bracket a kernel launch with profiling events when enabled.
struct ww_launch_scope {
  ww_ctx *ctx;
  const char *name;
  hipEvent_t a = nullptr, b = nullptr;
  ww_launch_scope(ww_ctx *c, const char *n) : ctx(c), name(n) {
    if (ctx->profiling) {
      hipEventCreate(&a);
      hipEventCreate(&b);
      hipEventRecord(a, ctx->stream);
    }
  }
  ~ww_launch_scope() {
    if (ctx->profiling) {
      hipEventRecord(b, ctx->stream);
      auto &e = ctx->prof[name];
      e.calls++;
      e.pending.emplace_back(a, b);
    }
  }
};

// A call's launch tables (launch_plan.h: ww_table_block; ww_bump is there too) and their way to the device.  send() takes the
// next of the context's two page-locked slots - waiting for the slot's event if its last copy is still in flight, growing it on
// demand -, packs the block there, enqueues ONE copy to d_block (bytes() bytes of device memory) on the context's stream and
// records the slot's event.  When it returns every registered array may be freed or overwritten, and the call has waited for no
// kernel (but where the slot has to grow: ww_ensure): a _dev entry point never synchronises for its tables.
struct ww_tables : ww_table_block {
  int send(ww_ctx *ctx, void *d_block) const;  // api.hip
};

// A tick's posteriors as {value, tick number} pairs in page-locked host memory, each written with ONE 8-byte store by the head
// of the model kernels (crnn.hip: cf_phases_d_to_g; wavenet.hip): the host polls them instead of waiting for the runtime's
// completion signal (streams.hip: ww_stream_step; 5.6 us of wake-up on this box, tools/launch_probe.hip).  slots == nullptr: off.
struct ww_tick_tag {
  unsigned long long *slots;  // [windows of the launch]: value bits | (uint64) seq << 32
  unsigned seq;
  int pidx;                   // the head's output element that is the posterior
};
#ifdef __HIPCC__
// One 8-byte store straight to page-locked host memory (system scope: not parked in L2): the host sees value and tick number
// together or not at all.
__device__ __forceinline__ void tick_tag_store(const ww_tick_tag &t, int w, float v, int k = 0) {
  // slot w + k (two indices: a kernel whose slot is base + row keeps the two pointer additions it had)
  const unsigned long long word = (unsigned long long)__float_as_uint(v) | ((unsigned long long)t.seq << 32);
  __hip_atomic_store(t.slots + w + k, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The same store for a value that is 32 bits of its own (stream_ctc.h: a streamed window's decode), not a float's
__device__ __forceinline__ void tick_tag_store(const ww_tick_tag &t, int w, unsigned bits) {
  const unsigned long long word = (unsigned long long)bits | ((unsigned long long)t.seq << 32);
  __hip_atomic_store(t.slots + w, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
#endif

struct ww_tick_fe;  // the streaming front end's side of a one-launch tick (stream_fe.h)

// ---- kernel-side entry points implemented in the .hip files ------------------------------
int ww_k_logmel(ww_ctx *ctx, const ww_model *m, const int16_t *d_pcm, const float *d_f32, const int64_t *d_sample_offs,
                const int64_t *d_frame_offs, int n_utt, int64_t total_frames, int64_t max_frames_per_utt,
                const ww_frontend_params *fp, float *d_mel, int64_t uniform_samples = 0,  // > 0: equal clips back to back from sample 0
                int64_t total_samples_hint = 0);  // > 0: sample_offs[n_utt], where the host knows it (device tables otherwise)
int ww_k_stft_mag(ww_ctx *ctx, const ww_model *m, const float *d_frames, int64_t n, int precise, float *d_mag);
int ww_k_mel_only(ww_ctx *ctx, const ww_model *m, const float *d_mag, int64_t n, float *d_mel);
int ww_k_crnn_detect(ww_ctx *ctx, const ww_model *m, const float *d_enc, int nw, float *d_out);
int ww_k_wave_detect(ww_ctx *ctx, const ww_model *m, const float *d_enc, int nw, float *d_out);
int ww_k_viterbi2(ww_ctx *ctx, const float *d_in, int64_t n, int T, float stay_bonus, int in_is_cost, unsigned char *d_path,
                  unsigned char *d_wake);

// `sliding`: the caller may pass regular sliding windows (row0 + w*hop), for which the scratch of crnn_rows_kernel is reserved too
size_t ww_crnn_workspace(const ww_model *m, int n_windows, bool sliding = true);
int ww_k_crnn_init_device(ww_ctx *ctx);  // per-device kernel attributes (dynamic LDS above 64 KB)
// ws_bytes: capacity of ws; a launch form that needs more (the model's options may have changed since ws was sized) fails with
// WW_EINVAL instead of writing past it
int ww_k_crnn_forward(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                      const int32_t *d_win_valid, int64_t row0, int hop, int valid_const, int n_windows, void *ws, size_t ws_bytes,
                      float *d_out, float *d_enc, const ww_tick_tag *tag = nullptr, const ww_set_ref *set = nullptr);
bool ww_crnn_segments_capable(const ww_model *m, int hop);
// a set's call of the sliding form (m: the set's view): ids: the call's member slots, a HOST array of n_ids checked ids; W: windows
// per member of the call; d_out: [n_ids][W][n_out].  Per group of sequences ONE crnn_rows_kernel<SET> and ONE tail launch over all slots
struct ww_crnn_set_call {
  long long stride;
  const int32_t *ids;
  int n_ids;
  int64_t W;
};
bool ww_crnn_set_segments_rows_form(const ww_model *m, int hop, int64_t W);
int ww_k_crnn_segments_forward(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *seg_row0,
                               const int32_t *seg_nw, int n_seg, int hop, float *d_out, const ww_crnn_set_call *set = nullptr);
bool ww_crnn_stream_capable(const ww_model *m);
int ww_k_crnn_stream_forward(ww_ctx *ctx, const ww_model *m, const float *d_hist, int64_t hist_rows, const int64_t *d_win_row,
                             const int32_t *d_win_valid, const int32_t *d_win_aux, float *d_gxc, int n_windows, float *d_out,
                             const ww_tick_tag *tag = nullptr, const ww_set_ref *set = nullptr);
// one launch per tick: front end + incremental CRNN of all S streams (2 S workgroups); posteriors as tags only.  every_k > 0: every
// stream runs every_k member slots (stream_all.h): 2 S every_k workgroups, set->ids and d_gxc by virtual stream, fe by physical
int ww_k_crnn_tick(ww_ctx *ctx, const ww_model *m, const ww_tick_fe &fe, int precise, float *d_gxc, const ww_tick_tag &tag,
                   const ww_set_ref *set = nullptr, int every_k = 0);
// does a ww_k_crnn_forward launch of n explicit windows write the tags (the one-kernel forms do)?
bool ww_crnn_forward_tags(const ww_model *m, int n_windows);
// CTC-trained CRNNs (WW_HEAD_CTC; crnn.hip).  ww_crnn_refuse_ctc: WW_EINVAL naming the ww_ctc_* family if m is one, WW_OK otherwise -
// the first statement of every launcher above and of the entry points that would do other work before they reach one.
// ww_crnn_ctc_check: the other way round (not a CTC CRNN, or one in split-bf16 mode: WW_EINVAL).
int ww_crnn_refuse_ctc(ww_ctx *ctx, const ww_model *m, const char *what);
int ww_crnn_ctc_check(ww_ctx *ctx, const ww_model *m, const char *what);
size_t ww_crnn_ctc_workspace(const ww_model *m, int n_windows);  // n_windows >= 1
// crnn_fused_kernel<front> + gru_tail_ctc_kernel, for explicit and for sliding windows;
// d_steps [n][19][L] and d_enc [n][19][64] may be nullptr
int ww_k_crnn_ctc_forward(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                          const int32_t *d_win_valid, int64_t row0, int hop, int valid_const, int n_windows, void *ws, size_t ws_bytes,
                          int max_labels, int32_t *d_labels, int32_t *d_lengths, float *d_steps, float *d_enc);
int ww_k_ctc_greedy(ww_ctx *ctx, const float *d_steps, int64_t n, int T, int L, int max_labels, int32_t *d_labels, int32_t *d_lengths);
// ctc_score_kernel (ctc_score.hip; the statement: ctc_score.h): the forward-algorithm score of K targets over any device posteriors
// [n][T][L], score[k * stride_k + i * stride_i] for sequence i and target k.  The targets travel as a kernel argument; a caller
// fills the struct only from arguments that ww_ctc_score_args_ok has passed (labels < 63 fit its bytes).
struct ww_ctc_score_targets {
  int8_t c[8][9];  // [WW_CTC_SCORE_MAX_TARGETS][WW_CTC_SCORE_MAX_TARGET]
  int8_t len[8];
  int32_t K = 0, mode = 0;
};
int ww_k_ctc_score(ww_ctx *ctx, const float *d_steps, int64_t n, int T, int L, const ww_ctc_score_targets &tg, float *d_score, int64_t stride_k,
                   int64_t stride_i);
// ctc_align_kernel (ctc_align.hip; the statement: ctc_align.h): the Viterbi alignment of the same K targets over the same posteriors.
// At o = k * stride_k + i * stride_i: d_value[o] and the 18 bytes d_span[18 o ..] ([WW_CTC_SCORE_MAX_TARGET][2] int8).
int ww_k_ctc_align(ww_ctx *ctx, const float *d_steps, int64_t n, int T, int L, const ww_ctc_score_targets &tg, float *d_value, int8_t *d_span,
                   int64_t stride_k, int64_t stride_i);
// ctc_occupancy_kernel (ctc_occupancy.hip; the statement: ctc_occupancy.h): the forward-backward occupancy of the same K targets over
// the same posteriors.  At o = k * stride_k + i * stride_i: d_value[o], d_occ[o][T][WW_CTC_SCORE_MAX_TARGET] and, where d_cls is not
// nullptr (exact mode only), d_cls[o][T][L].  The arguments have passed ww_ctc_occupancy_args_ok.
int ww_k_ctc_occupancy(ww_ctx *ctx, const float *d_steps, int64_t n, int T, int L, const ww_ctc_score_targets &tg, float *d_value, float *d_occ,
                       float *d_cls, int64_t stride_k, int64_t stride_i);
// ctc_beam_kernel (ctc_beam.hip; the statement: ctc_beam.h): the prefix beam search over any device posteriors [n][T][L], a wave per
// sequence: d_labels [n][P][max_labels], d_lengths [n][P], d_prob [n][P].  The arguments have passed ww_ctc_beam_args_ok.
int ww_k_ctc_beam(ww_ctx *ctx, const float *d_steps, int64_t n, int T, int L, int W, int P, int max_labels, int32_t *d_labels, int32_t *d_lengths,
                  float *d_prob);
// A CTC stream bank's incremental ticks (crnn_stream_kernel<FE, false, false, CTC>): ww_k_crnn_tick's and ww_k_crnn_stream_forward's
// arguments; a window's decode goes out as one 32-bit word (stream_ctc.h) - the value half of its tag where tag slots are given, else
// row w of d_words -, and with d_steps (page-locked, [windows of the launch][19][L]; nullptr: off) its posteriors beside it
int ww_k_crnn_ctc_tick(ww_ctx *ctx, const ww_model *m, const ww_tick_fe &fe, int precise, float *d_gxc, const ww_tick_tag &tag, float *d_steps);
int ww_k_crnn_ctc_stream_forward(ww_ctx *ctx, const ww_model *m, const float *d_hist, int64_t hist_rows, const int64_t *d_win_row,
                                 const int32_t *d_win_valid, const int32_t *d_win_aux, float *d_gxc, int n_windows, uint32_t *d_words,
                                 float *d_steps, const ww_tick_tag *tag = nullptr);
size_t ww_wave_workspace(const ww_model *m, int n_windows);
int ww_k_wave_forward(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                      const int32_t *d_win_valid, int64_t row0, int hop, int valid_const, int n_windows, void *ws, size_t ws_bytes,
                      float *d_out, float *d_enc, const ww_tick_tag *tag = nullptr, const ww_set_ref *set = nullptr);
// the five passes of ww_posterior_events over device posteriors; ws: p.bytes of device scratch with offsets and thresholds in place
int ww_k_posterior_events(ww_ctx *ctx, const float *d_post, const ev_plan &p, int win, char *ws);
int ww_k_posterior_pick(ww_ctx *ctx, const float *d_rows, int64_t n, int n_out, int pidx, const int64_t *d_seg_offs, int64_t n_seg,
                        float *d_out);
bool ww_wave_tick_capable(const ww_model *m, int n_streams);
int ww_k_wave_tick(ww_ctx *ctx, const ww_model *m, const ww_tick_fe &fe, int precise, const ww_tick_tag &tag, const ww_set_ref *set = nullptr);
// The fp32 Wavenet's sequence form (wavenet.hip: wavenet_seq_kernel) over launch_plan.h's segments (wv_seg).
int ww_wave_receptive_field(const ww_model *m);  // 1 + 2 * sum of the dilations
// the form's reach, for the entry point or launcher `what`: WW_EINVAL for a CRNN and for a model in split-bf16 mode
int ww_wave_seq_check(ww_ctx *ctx, const ww_model *m, const char *what);
// set (m: the set's view): segments x planes workgroups in ONE launch, enc / logits [planes][plane_rows][...]; the member of plane y is
// set->ids[y], or - set->aux given, one plane - the member of segment x is set->ids[set->aux[x]] (launch_plan.h: seg_seq)
int ww_k_wave_sequence(ww_ctx *ctx, const ww_model *m, const float *d_mel, const wv_seg *d_segs, int n_segs, float *d_enc, float *d_logits,
                       const ww_set_ref *set = nullptr, int planes = 1, int64_t plane_rows = 0);
// rows = offs[n_seq] - offs[0] (the rows that belong to a sequence), row_end = offs[n_seq]; planes of plane_rows rows: as above
int ww_k_wave_pool(ww_ctx *ctx, const float *d_z, int64_t rows, int64_t row_end, int n_out, const int64_t *d_offs, int n_seq, int64_t pool_rows,
                   int64_t max_len, float *d_a, float *d_b, float *d_pf, float *d_post, int planes = 1, int64_t plane_rows = 0);
#define WW_WAVE_STATE_BLOCK 256  // floats of carried state per block and stream: [4 channel groups][16 rows][4]
// A causal bank's feed (streams.hip: ww_stream_feed) over launch_plan.h's tables (wv_feed_seg, wv_feed_pool):
// segs[0, n_small): one-wave form (posteriors, ring and state inside the kernel); segs[n_small, n_segs): twelve-wave form, logits to
// d_z, then pool[n_pool] -> d_post and ring[n_ring] (one entry per such stream) -> the logit rings
int ww_k_wave_feed(ww_ctx *ctx, const ww_model *m, const float *d_rows, const wv_feed_seg *d_segs, int n_small, int n_segs,
                   const wv_feed_pool *d_pool, int n_pool, const wv_feed_pool *d_ring, int n_ring, float *d_z, float *d_state,
                   float *d_zring, int32_t *d_zpos, int pidx, float *d_post, const ww_set_ref *set = nullptr, int slots = 0,
                   int64_t plane_rows = 0, float *d_post_rows = nullptr);
int ww_k_wave_stream_tick(ww_ctx *ctx, const ww_model *m, const float *d_hist, const int64_t *d_win_row, const int32_t *d_win_valid,
                          const int32_t *d_win_aux, int nw, float *d_state, float *d_zring, int32_t *d_zpos, float *d_out,
                          const ww_tick_tag *tag, const ww_set_ref *set = nullptr);
// A stream bank at other rates than 16 kHz (resample.hip; geometry and bookkeeping: stream_rate.h, stream_rates.h).  ONE state
// object, which belongs to the bank (streams.hip) and borrows the resamplers' tap tables: rs[k] = rate class k (nullptr: the 16 kHz
// class), stream_rate[s] = the class of stream s (nullptr: all 0).  `uniform` (ww_stream_attach_resampler): the one class rs[0], every
// stream in it for good, frames [S][F] - _frame_samples gives F there and 0 on a per-stream bank, whose frames are one ragged block
// (_layout).  _create: WW_EINVAL with the refusal's reason.  _tick: the frames -> the [S][320] int16 device block *d_frames that the
// tick's kernels then read, ONE kernel for every class on the context's stream in front of them; flags = the tick's (bit 1: the
// stream is frozen), ctl_dev = the tick's control words as the device sees them.  _reset: the listed streams' counts to 0 (ids ==
// nullptr: streams 0 .. count - 1).  _move: the listed streams to class c with their counts at 0, the device table behind it in
// stream order.  _advance: the 16 kHz samples `stream` would consume on k more input samples (no state moves).  _feed: the call's
// 16 kHz samples into d_dst (see resample.hip).
struct ww_resampler;
struct ww_stream_rates;
// formats[k] (nullptr: all int16) = the sample format class k reads its frames and packets in (stream_formats.h): with a G.711 class
// in the bank (_g711) a tick's frames are one BYTE block (_layout_bytes; a uniform bank: [S][F] of the format) and a feed's packets
// are counted in bytes.  `what`: the entry point's name, for the refusals.
int ww_k_rates_create(ww_ctx *ctx, const ww_resampler *const *rs, const int32_t *formats, int n_rates, const int32_t *stream_rate, int S, bool uniform,
                      const char *what, ww_stream_rates **out);
bool ww_k_rates_g711(const ww_stream_rates *rt);
int ww_k_rates_stream_format(const ww_stream_rates *rt, int stream);
void ww_k_rates_layout_bytes(const ww_stream_rates *rt, int32_t *frame_bytes, int64_t *byte_offs, int32_t *formats);  // [S], [S + 1], [S]; each may be nullptr
void ww_k_rates_destroy(ww_stream_rates *rt);
int ww_k_rates_classes(const ww_stream_rates *rt);
int ww_k_rates_frame_samples(const ww_stream_rates *rt);
void ww_k_rates_layout(const ww_stream_rates *rt, int32_t *frame_samples, int64_t *frame_offs);  // [S], [S + 1]; either may be nullptr
void ww_k_rates_reset(ww_stream_rates *rt, const int32_t *ids, int count);
int ww_k_rates_move(ww_stream_rates *rt, const int32_t *ids, int count, int c);
int64_t ww_k_rates_advance(const ww_stream_rates *rt, int stream, int64_t k);
int ww_k_rates_tick(ww_stream_rates *rt, const int16_t *frames, const uint8_t *flags, const int32_t *ctl_dev, const int16_t **d_frames);
int ww_k_rates_feed(ww_stream_rates *rt, const int32_t *ids, int n, const void *data, const int64_t *byte_offs, const int64_t *offs16,
                    int16_t *d_dst, bool *moved);
int ww_k_far_frr(ww_ctx *ctx, const float *d_pos, int64_t n_pos, const float *d_neg, int64_t n_neg, int win,
                 const double *d_thr, int n_thr, double *d_smoothed, unsigned long long *d_pos_cnt,
                 unsigned long long *d_fa_cnt);

// streaming CRNN: slots of the per-stream ring of projected rows (crnn.hip, crnn_stream_kernel): a row written for the window
// that ends at stream row r is last read by the window that ends at r + 128, and overwritten at r + WW_STREAM_GXC
#define WW_STREAM_GXC 144

#ifdef __HIPCC__
// A SET kernel's first steps: the member id as a scalar (the index is uniform over the workgroup; readfirstlane says so where the
// compiler cannot see it), and a weight pointer moved on to that member's block - scalar arithmetic, once per workgroup.
__device__ __forceinline__ long long ww_set_offset(const ww_set_ref &set, int i) {
  return (long long)__builtin_amdgcn_readfirstlane(set.ids[i]) * set.stride;
}
template <typename T>
__device__ __forceinline__ void ww_set_move(const T *&p, long long off) {
  p = (const T *)((const char *)p + off);
}

// max(x, 0) as ONE instruction: fmaxf compiles to a canonicalising v_max (x, x) in front of the v_max (0, x) when its
// argument comes out of an MFMA.  On the bit pattern a signed-integer max does the same job (negative floats, -0
// included, are negative integers).  Not inline asm: the compiler does not see an MFMA -> VALU read hazard through it
// and omits the wait states.
// Pre-emphasis x - a * b as the reference computes it: two fp32 operations, the product rounded before the subtraction
// (NumPy float32).  __fmul_rn / __fsub_rn are plain * and - in these headers, which the compiler contracts into one FMA (one
// rounding: an ulp off a sample, up to 5e-4 in the log-mel of bands far below their frame's 2-norm).
__device__ __forceinline__ float ww_preemph_rn(float x, float a, float b) {
#pragma clang fp contract(off)
  const float p = a * b;
  return x - p;
}

__device__ __forceinline__ float relu1(float x) {
  const int b = __float_as_int(x);
  return __int_as_float(b > 0 ? b : 0);
}
#endif
