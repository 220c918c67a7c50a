// stream_rates.h - the host-only geometry of a stream bank whose streams each run at their own sample rate (include/wwhip.h:
// ww_stream_attach_rates).  Plain C++ on top of stream_rate.h (no HIP header, no HIP call): common.h includes it
// for the .hip files, and tests/native/stream_rates_check.cpp compiles it alone under Address + UB sanitizer on the CPU.
//
// A bank has up to WW_STREAM_MAX_RATES rate classes; stream s belongs to class cls[s] and is, in every respect, a stream of the
// single-rate bank of that class (stream_rate.h): the same rate_geom, the same rate_advance, the same control words.  The 16 kHz
// class is a pass-through: 320 samples per tick that go into the tick's block as they are, no delay, no history, no count.
// What is new is what follows from streams of different classes sharing one tick: the ragged layout of a tick's frames, the LDS
// the tick's kernel asks for, a stream's move to another class, and the grouping of a feed's packets by class.
#pragma once

#include <cstring>
#include <vector>

#include "stream_rate.h"

#ifndef WW_STREAM_MAX_RATES
#define WW_STREAM_MAX_RATES 8
#endif

struct rates_table {
  int K = 0;
  rate_geom g[WW_STREAM_MAX_RATES];
  bool pass[WW_STREAM_MAX_RATES] = {};  // the 16 kHz class
};

// the 16 kHz class as a geometry: a frame of 320 samples, one sample in for one sample out, nothing in front and nothing kept
static inline rate_geom rates_pass_geom() {
  rate_geom g;
  g.rate_in = WW_RATE_OUT;
  g.F = WW_RATE_FRAME_OUT;
  return g;
}

// The next class of a table: a resampler's (up, down, half, tpp) for rate_in -> rate_out, or with pass = true the 16 kHz class (the
// other arguments are not looked at).  1 and "class <k>: <reason>" in `why`, or 0.  The refusals of a class on its own are
// rate_make_geom's; those of a class among the others: a ninth class, a second 16 kHz class, an input rate the table already has.
static inline int rates_add_class(rates_table &t, bool pass, int32_t rate_in, int32_t rate_out, int64_t up, int64_t down, int64_t half, int64_t tpp,
                                  char *why, size_t cap) {
  const int k = t.K;
  if (k >= WW_STREAM_MAX_RATES) {
    snprintf(why, cap, "class %d: a bank has at most %d rate classes", k, WW_STREAM_MAX_RATES);
    return 1;
  }
  rate_geom g = rates_pass_geom();
  if (!pass) {
    char reason[200];
    if (rate_make_geom(rate_in, rate_out, up, down, half, tpp, g, reason, sizeof reason)) {
      snprintf(why, cap, "class %d: %s", k, reason);
      return 1;
    }
  }
  for (int j = 0; j < k; ++j) {
    if (pass && t.pass[j]) {
      snprintf(why, cap, "class %d: class %d is the 16 kHz class already (one NULL class per bank)", k, j);
      return 1;
    }
    if (t.g[j].rate_in == g.rate_in) {
      snprintf(why, cap, "class %d: %d Hz is class %d's rate already (two classes of the same input rate)", k, g.rate_in, j);
      return 1;
    }
  }
  t.g[k] = g;
  t.pass[k] = pass;
  t.K = k + 1;
  return 0;
}

// cls[i] in [0, K) for every i < n (cls == nullptr: all class 0); 1 and the index in `why` otherwise
static inline int rates_check_ids(const rates_table &t, const int32_t *cls, int64_t n, const char *what, char *why, size_t cap) {
  for (int64_t i = 0; cls && i < n; ++i)
    if (cls[i] < 0 || cls[i] >= t.K) {
      snprintf(why, cap, "%s[%lld] = %d: the bank has rate classes 0..%d", what, (long long)i, cls[i], t.K - 1);
      return 1;
    }
  return 0;
}

// A tick's frames: ONE ragged int16 block, stream s's F(cls[s]) samples from sample frame_offs[s], nothing between the streams.
// frame_samples [S] and frame_offs [S + 1] may each be nullptr; -> the block's samples (= frame_offs[S]).
static inline int64_t rates_layout(const rates_table &t, const int32_t *cls, int S, int32_t *frame_samples, int64_t *frame_offs) {
  int64_t at = 0;
  for (int s = 0; s < S; ++s) {
    const int F = t.g[cls[s]].F;
    if (frame_samples) frame_samples[s] = F;
    if (frame_offs) frame_offs[s] = at;
    at += F;
  }
  if (frame_offs) frame_offs[S] = at;
  return at;
}

// the block's samples at most, whatever the streams move to: what a bank reserves once
static inline int64_t rates_layout_max(const rates_table &t, int S) {
  int F = 0;
  for (int k = 0; k < t.K; ++k) F = t.g[k].F > F ? t.g[k].F : F;
  return (int64_t)S * F;
}

// The floats one workgroup of the tick's kernel stages: the largest [history | frame | pad] of the bank's resampling classes (the
// 16 kHz class stages nothing).  1 and the reason above WW_RATE_STAGE_MAX (no class rate_make_geom accepted gets there; a table put
// together by other means might).
static inline int rates_stage(const rates_table &t, int64_t *floats, char *why, size_t cap) {
  int64_t m = 0;
  for (int k = 0; k < t.K; ++k) {
    if (t.pass[k]) continue;
    const int64_t n = (int64_t)t.g[k].hist + t.g[k].F + WW_RATE_PAD;
    if (n > WW_RATE_STAGE_MAX) {
      snprintf(why, cap, "class %d: %d Hz needs %lld staged samples per tick; the tick stages %d at most", k, t.g[k].rate_in, (long long)n,
               WW_RATE_STAGE_MAX);
      return 1;
    }
    m = n > m ? n : m;
  }
  *floats = m;
  return 0;
}

// the 16 kHz samples a stream of class c with n inputs so far consumes on k more (the 16 kHz class: k)
static inline int64_t rates_advance(const rates_table &t, int c, int64_t n, int64_t k) { return t.pass[c] ? k : rate_advance(t.g[c], n, k).count; }

// A tick of a stream of class c that is not frozen: its control words - those of the single-rate bank of that class at the same
// count - and the count moves on by the class's frame.  (The 16 kHz class has neither: zeros, and n stays 0.)
static inline rate_ctl rates_tick(const rates_table &t, int c, int64_t &n) {
  rate_ctl rc = {0, 0, 0, 0};
  if (t.pass[c]) return rc;
  const rate_step st = rate_advance(t.g[c], n, t.g[c].F);
  rc.res = st.res;
  rc.zeros = (int32_t)st.zeros;
  rc.held = st.held;
  n += t.g[c].F;
  return rc;
}

// A stream moves to class c, or is reset: the next sample is x[0] of a new signal.  With the count at 0 its `held` is 0, and every
// sample of its history row - whichever class wrote it - reads as zero: no kernel clears anything.
static inline void rates_move(int32_t &cls, int64_t &n, int c) {
  cls = c;
  n = 0;
}

// The tick's per-stream descriptor (a DEVICE table the bank resends when a stream moves)
struct rates_desc {
  int64_t off;  // the frame's first BYTE in the tick's block (2 x its first sample in a bank of int16 frames; stream_formats.h)
  int32_t cls, pad;
};

// A feed's packets by class: order[start[c] .. start[c + 1]) are the indices i of the call's packets with pkt_cls[i] == c, ascending
// - a partition of 0 .. n - 1 that keeps each class's packets in the call's order.
struct rates_groups {
  std::vector<int32_t> order;
  int32_t start[WW_STREAM_MAX_RATES + 1] = {};
};
static inline void rates_group(const int32_t *pkt_cls, int n, rates_groups &g) {
  memset(g.start, 0, sizeof g.start);
  for (int i = 0; i < n; ++i) ++g.start[pkt_cls[i] + 1];
  for (int c = 0; c < WW_STREAM_MAX_RATES; ++c) g.start[c + 1] += g.start[c];
  g.order.assign((size_t)n, 0);
  int32_t at[WW_STREAM_MAX_RATES];
  for (int c = 0; c < WW_STREAM_MAX_RATES; ++c) at[c] = g.start[c];
  for (int i = 0; i < n; ++i) g.order[(size_t)at[pkt_cls[i]]++] = i;
}
