// stream_all.h - the host-only half of a stream bank's tick (streams.hip: stream_step_impl), and of the bank that runs EVERY listed
// member of a model set on EVERY stream (include/wwhip.h: ww_stream_create_set_all).  Plain C++ (no HIP header, no HIP call):
// csrc/streams.hip includes it; tests/native/stream_all_check.cpp compiles it alone under Address + UB sanitizer on the CPU
// (tests/test_stream_all_host.py).
//
// A bank of S streams and K member slots has S * K VIRTUAL streams: v = s * K + j is member slot j on physical stream s.  Everything
// the model side keeps per stream - the member table the SET kernels read (ids[v]), the CRNN's cache of projected rows, the causal
// state and logit ring, the tag slots - is indexed by v; everything the front end keeps - the sample ring, the pre-emphasis carry,
// the mirrored mel ring, the control words, the frames - by s = v / K.  An ordinary bank is the K = 1 case: v = s.
//
// One tick of one physical stream (sa_tick_stream) is the integer bookkeeping of spokestack/wakeword/tflite.py:163-168 - how many
// frames the tick completes, how many posteriors it owes - and what the tick's kernels are told about it, by launch form:
//   SA_ONE_LAUNCH  the control words only: workgroup 2 v + k finds everything else out by itself; its posterior arrives in tag slot
//                  2 v + k
//   SA_CAUSAL      one descriptor per virtual stream with new rows: row = s * HR + pos (physical), valid = the new rows,
//                  aux = v | emit << 16; posteriors in slot 2 v + k
//   SA_TABLE       one descriptor per window (incremental CRNN in two launches, Wavenet window bank): row = s * HR + first slot of
//                  the window's block (physical), valid = T, aux = v * gxc + the window's slot of v's cache ring; the posterior of
//                  descriptor i arrives in slot i.  Descriptors run in (s, j, k) order
// and sa_scatter puts what arrived where the caller reads it: post[s][j][k], zeros beyond n_post[s].
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/wwhip.h"

#define WW_ALL_MAX_MEMBERS 64    // member slots of an every-member bank
#define WW_ALL_MAX_VIRTUAL 65535  // S * K: the causal descriptor keeps the virtual stream in 16 bits

enum sa_form { SA_ONE_LAUNCH = 0, SA_CAUSAL = 1, SA_TABLE = 2 };

static inline int sa_refuse(char *err, size_t cap, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
static inline int sa_refuse(char *err, size_t cap, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  if (err && cap) vsnprintf(err, cap, fmt, ap);
  va_end(ap);
  return WW_EINVAL;
}

// ---- virtual streams --------------------------------------------------------------------------------------------------------------
static inline int sa_virtual(int s, int K, int j) { return s * K + j; }
static inline int sa_stream(int v, int K) { return v / K; }
static inline int sa_slot(int v, int K) { return v % K; }

// May a bank of S streams run K member slots on each, under these creation flags?  WW_OK, or WW_EINVAL with the reason in err.
// (The member ids themselves are ww_set_check_ids's, model_set.h.)
static inline int sa_check_create(int64_t S, int64_t K, uint32_t flags, char *err, size_t cap) {
  if (K < 1 || K > WW_ALL_MAX_MEMBERS) return sa_refuse(err, cap, "%lld member slots: an every-member bank has 1..%d", (long long)K, WW_ALL_MAX_MEMBERS);
  if (flags & WW_STREAM_FULL_RECOMPUTE)
    return sa_refuse(err, cap, "WW_STREAM_FULL_RECOMPUTE runs the per-window batch kernels: not offered on a model set");
  if (flags & ~(uint32_t)(WW_STREAM_TWO_LAUNCH | WW_STREAM_SYNC_WAIT | WW_STREAM_CAUSAL)) return sa_refuse(err, cap, "unknown stream flags 0x%x", flags);
  if (S < 1) return sa_refuse(err, cap, "stream count %lld out of range", (long long)S);
  if (S * K > WW_ALL_MAX_VIRTUAL)
    return sa_refuse(err, cap, "%lld streams x %lld member slots = %lld virtual streams: a bank has at most %d", (long long)S, (long long)K,
                     (long long)(S * K), WW_ALL_MAX_VIRTUAL);
  return WW_OK;
}

// The member table the SET kernels read: ids[v] = members[v % K]; members == nullptr: every member in order (slot j = member j).
static inline void sa_member_table(const int32_t *members, int K, int S, std::vector<int32_t> &ids) {
  ids.resize((size_t)S * K);
  for (int s = 0; s < S; ++s)
    for (int j = 0; j < K; ++j) ids[(size_t)sa_virtual(s, K, j)] = members ? members[j] : j;
}

// Which calls an every-member bank takes and which an ordinary bank takes.  `every` = the bank was created by
// ww_stream_create_set_all; `call` = the entry point's name; `wants_every` = the call is one of that bank's own (ww_stream_step_all,
// ww_stream_feed_all, ww_stream_feed_rows_all, ww_stream_step_trigger_all).  WW_OK, or WW_EINVAL
// with the reason in err - looked at before any state moves.
static inline int sa_check_call(bool every, const char *call, bool wants_every, char *err, size_t cap) {
  if (every && !wants_every)
    return sa_refuse(err, cap, "%s: this bank runs every listed member on every stream (ww_stream_create_set_all): its tick is ww_stream_step_all, "
                     "its feed ww_stream_feed_all, its trigger stage ww_stream_step_trigger_all, and it has no per-stream member", call);
  if (!every && wants_every) return sa_refuse(err, cap, "%s: this bank was not created by ww_stream_create_set_all: its tick is ww_stream_step", call);
  return WW_OK;
}

// The id list of ww_stream_reset, ww_stream_set_model and ww_stream_set_rate on a bank of S streams: ids == nullptr names every stream
// (n is not looked at); else n ids, a stream as often as the caller likes, up to the 2 S entries the list is staged in.  WW_OK, or
// WW_EINVAL with the reason in err, looked for in this order: a negative count, more ids than that, an id out of range.
static inline int sa_check_ids(const int32_t *ids, int64_t n, int S, char *err, size_t cap) {
  if (!ids) return WW_OK;
  if (n < 0) return sa_refuse(err, cap, "negative id count");
  if (n > 2 * (int64_t)S) return sa_refuse(err, cap, "more ids than streams");
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= S) return sa_refuse(err, cap, "stream id %d out of range", (int)ids[i]);
  return WW_OK;
}

// ---- one tick ---------------------------------------------------------------------------------------------------------------------
// frames that `tot` buffered samples complete (one whenever `window` are buffered, then the oldest `hop` are dropped): the rule of
// stream_fe.h's ww_fe_frames, which the feed uses, stated where no HIP header is in reach (the check program holds it against the
// reference's sample-by-sample loop)
static inline int sa_frames(int64_t tot, int window, int hop) { return tot >= window ? (int)((tot - window) / hop) + 1 : 0; }

struct sa_tick {
  // the bank
  int S = 0, K = 1;
  int T = 0, HR = 0;          // the model's window rows; rows of a stream's mirrored mel ring = 2 (T + 1)
  int hop = 160, chunk = 320, window = 512;
  int gxc = 0;                // slots of a virtual stream's ring of projected rows (WW_STREAM_GXC)
  sa_form form = SA_TABLE;
  // the host's mirrors of the streams' state, [S]: samples pending, mel rows written (mod T + 1), rows since the reset (mod gxc),
  // state parity (one-launch form)
  int *fill = nullptr, *pos = nullptr, *rowq = nullptr, *par = nullptr;
  // what the tick's kernels read: control words [S][4]; descriptors [2 S K]
  int32_t *ctl = nullptr;
  int64_t *row = nullptr;
  int32_t *valid = nullptr, *aux = nullptr;
  std::vector<int> *expect = nullptr;  // tag slots this tick's posteriors arrive in
  int nw = 0, nd = 0;                  // posteriors of the tick (over all slots) | descriptors written
};

// Physical stream s of the tick, flags bit 0 = is_speech, bit 1 = is_active: the control words, the descriptors and tag slots of its K
// virtual streams, and the mirrors advanced.  Returns the posteriors per member slot the tick owes for it (0, 1 or 2).
static inline int sa_tick_stream(sa_tick &t, int s, int flags) {
  flags &= 3;
  const int R = t.T + 1, K = t.K;
  const int nf = (flags & 2) ? 0 : sa_frames((int64_t)t.fill[s] + t.chunk, t.window, t.hop);
  const int np = (flags & 1) && !(flags & 2) ? nf : 0;
  int32_t *cw = t.ctl + (size_t)s * 4;
  cw[0] = t.fill[s];
  cw[1] = nf;
  if (t.form == SA_ONE_LAUNCH) {
    cw[2] = flags | (t.par[s] << 2);
    cw[3] = t.pos[s] | (t.rowq[s] << 16);
    for (int j = 0; j < K; ++j)
      for (int k = 0; k < np; ++k) t.expect->push_back(2 * sa_virtual(s, K, j) + k);
    if (!(flags & 2)) t.par[s] ^= 1;
  } else if (t.form == SA_CAUSAL) {
    // every sampled row is analysed and advances the state; bit 0 only decides whether its posterior is emitted.  The new rows are
    // rows pos, pos + 1 of the stream's mirrored ring (contiguous: pos + 1 <= R)
    cw[2] = flags | 1;
    cw[3] = t.pos[s];
    for (int j = 0; j < K && nf; ++j) {
      const int v = sa_virtual(s, K, j);
      t.row[t.nd] = (int64_t)s * t.HR + t.pos[s];
      t.valid[t.nd] = nf;
      t.aux[t.nd] = v | ((np ? 1 : 0) << 16);
      ++t.nd;
      for (int k = 0; k < np; ++k) t.expect->push_back(2 * v + k);
    }
  } else {
    cw[2] = flags;
    cw[3] = t.pos[s];
    for (int j = 0; j < K; ++j) {
      const int v = sa_virtual(s, K, j);
      for (int k = 0; k < np; ++k) {
        // the T rows that end at this tick's new row k are the contiguous block that starts at (pos + k + 2) % R
        t.row[t.nd] = (int64_t)s * t.HR + (t.pos[s] + k + 2) % R;
        t.valid[t.nd] = t.T;
        t.aux[t.nd] = v * t.gxc + (t.rowq[s] + k + 1) % t.gxc;  // rows since the reset incl. this window's newest
        t.expect->push_back(t.nd);
        ++t.nd;
      }
    }
  }
  t.nw += np * K;
  if (!(flags & 2)) t.fill[s] = t.fill[s] + t.chunk - nf * t.hop;
  t.pos[s] = (t.pos[s] + (t.form == SA_CAUSAL ? nf : np)) % R;
  t.rowq[s] = (t.rowq[s] + np) % t.gxc;
  return np;
}

// The tick's posteriors where the caller reads them: post[s][j][k] = fetch(slot the posterior of (s, j, k) arrived in), zeros for
// k >= n_post[s].  The slots are sa_tick_stream's: 2 v + k, or in the table form the running descriptor index.
template <typename Fetch>
static inline void sa_scatter(sa_form form, int S, int K, const int32_t *n_post, Fetch &&fetch, float *post) {
  int w = 0;
  for (int s = 0; s < S; ++s)
    for (int j = 0; j < K; ++j) {
      float *p = post + (size_t)sa_virtual(s, K, j) * 2;
      p[0] = p[1] = 0.f;
      for (int k = 0; k < n_post[s]; ++k, ++w) p[k] = fetch(form == SA_TABLE ? w : 2 * sa_virtual(s, K, j) + k);
    }
}

// The virtual streams of a reset's ids: K per named stream (ids == nullptr: all), in the order named.
static inline void sa_virtual_ids(const int32_t *ids, int count, int K, std::vector<int32_t> &out) {
  out.resize((size_t)count * K);
  for (int i = 0; i < count; ++i)
    for (int j = 0; j < K; ++j) out[(size_t)i * K + j] = sa_virtual(ids ? ids[i] : i, K, j);
}

// ---- the trigger stage --------------------------------------------------------------------------------------------------------------
// spokestack/wakeword/tflite.py:134-146 (VAD edge, reset on the fall) and :232-239 (running maximum, threshold, activation) over the
// posteriors a tick delivered, per stream, with K member slots - the ONE statement of the rule: ww_trigger_bank_step and
// ww_stream_step_trigger are its K = 1 case (one threshold, fired_slot and fired_mask not asked for).
//   post [S][K][2], n_post [S] (0..2 rows of the tick), thresholds [K], posterior_max [S][K]
//   - posterior_max[s][j] is slot j's running maximum; all K are cleared on the VAD falling edge (behind this tick's rows)
//   - slot j EXCEEDS on a row when (double)p > thresholds[j]: the reference's float32 posterior against a Python float
//   - a stream that is not active FIRES when any slot exceeds on any row: is_active[s] = 1, once, and entry i of the three lists:
//     fired_ids[i] = s; fired_mask[i] bit j = slot j exceeded on some row of the tick; fired_slot[i] = the winner - on the earliest
//     row on which any slot exceeded, the exceeding slot with the greatest posterior, the lowest slot among equals
//   - a stream that is already active does not fire again (no entry); its maxima still move
//   - fall_ids: the streams whose VAD bit fell (the caller resets them)
// fired_slot / fired_mask may be nullptr (K = 1: they would be 0 and 1).  Arguments are the caller's to check.
static inline void sa_trigger_update(int S, int K, const uint8_t *is_speech, uint8_t *is_active, const float *post, const int32_t *n_post,
                                     const double *thresholds, uint8_t *was_speech, float *posterior_max, int32_t *fired_ids,
                                     int32_t *fired_slot, uint64_t *fired_mask, int32_t *n_fired, int32_t *fall_ids, int32_t *n_fall) {
  int nf = 0, nl = 0;
  for (int s = 0; s < S; ++s) {
    const uint8_t sp = is_speech[s] != 0;
    const bool fall = was_speech[s] && !sp;
    was_speech[s] = sp;
    const float *ps = post + (size_t)s * K * 2;
    float *pm = posterior_max + (size_t)s * K;
    uint64_t mask = 0;
    int win = -1;
    for (int k = 0; k < n_post[s]; ++k) {
      int best = -1;
      for (int j = 0; j < K; ++j) {
        const float p = ps[j * 2 + k];
        if (p > pm[j]) pm[j] = p;
        if ((double)p > thresholds[j]) {
          mask |= (uint64_t)1 << j;
          if (best < 0 || p > ps[best * 2 + k]) best = j;
        }
      }
      if (win < 0) win = best;
    }
    if (win >= 0 && !is_active[s]) {
      is_active[s] = 1;
      fired_ids[nf] = s;
      if (fired_slot) fired_slot[nf] = win;
      if (fired_mask) fired_mask[nf] = mask;
      ++nf;
    }
    if (fall) {
      for (int j = 0; j < K; ++j) pm[j] = 0.f;
      fall_ids[nl++] = s;
    }
  }
  *n_fired = nf;
  *n_fall = nl;
}

// The arguments of ww_trigger_bank_step_all (include/wwhip.h): WW_OK, or WW_EINVAL with the reason in err
static inline int sa_check_trigger(int64_t S, int64_t K, const void *is_speech, const void *is_active, const void *post, const int32_t *n_post,
                                   const void *thresholds, const void *was_speech, const void *posterior_max, const void *fired_ids,
                                   const void *fired_slot, const void *fired_mask, const void *n_fired, const void *fall_ids, const void *n_fall,
                                   char *err, size_t cap) {
  if (S < 0) return sa_refuse(err, cap, "stream count %lld out of range", (long long)S);
  if (K < 1 || K > WW_ALL_MAX_MEMBERS) return sa_refuse(err, cap, "%lld member slots: the trigger stage takes 1..%d", (long long)K, WW_ALL_MAX_MEMBERS);
  if (!n_fired || !n_fall || !thresholds) return sa_refuse(err, cap, "NULL argument");
  if (S > 0 && (!is_speech || !is_active || !post || !n_post || !was_speech || !posterior_max || !fired_ids || !fired_slot || !fired_mask || !fall_ids))
    return sa_refuse(err, cap, "NULL argument");
  for (int64_t s = 0; s < S; ++s)
    if (n_post[s] < 0 || n_post[s] > 2) return sa_refuse(err, cap, "n_post[%lld] = %d: a tick delivers 0..2 rows", (long long)s, (int)n_post[s]);
  return WW_OK;
}
