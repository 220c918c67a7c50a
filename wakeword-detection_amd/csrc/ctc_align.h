// ctc_align.h - the Viterbi alignment of a target over one window's per-step class posteriors: the most probable path through the
// target's CTC lattice, and the steps at which that path enters and leaves every label.  ctc_score.h's forward algorithm says
// WHETHER a window reads [HEY][SNIPS]; this says WHERE in the window each of the two lies, to one conv step - what the stage behind
// the wake word (an activation timeout, a recogniser that takes the audio after the word) needs first.  It is the max-product twin
// of that header's sum-product lattice, with back-pointers and a back-trace.  One definition for ctc_align_kernel (ctc_align.hip:
// the same operations, a lattice state per lane), ww_ctc_align_rows (api.hip: this function over host arrays) and the host check
// (tests/native/ctc_align_check.cpp).  Plain C++ that a device compiler also takes.  wwhip/ctc.py: align is the same in float64.
//
// y [T][L], the target c[0 .. U), the states s = 0 .. 2U, cls(s) and skip(s): ctc_score.h's, and so are the limits and the argument
// rule (ww_ctc_score_args_ok).
//   v_0(0) = y_0[blank], v_0(1) = y_0[c_0], every other state 0
//   t >= 1: the candidates in the order v_{t-1}(s) (shift 0), v_{t-1}(s - 1) (shift 1, s >= 1), v_{t-1}(s - 2) (shift 2, skip(s));
//   the best is the FIRST of the largest - start from shift 0, replace on a strict > only -; bp_t(s) is its shift and
//   v_t(s) = best * y_t[cls(s)]: one float32 multiplication (ww_cs_mul) per step, and nothing else rounds.
// WW_CTC_SCORE_EXACT - the path ends at T - 1 in state 2U - 1, or in 2U if v(2U) > v(2U - 1) strictly; the value is that v.
// WW_CTC_SCORE_PREFIX - the trigger's rule, what follows a completed target is free:
//   q_t = m * y_t[c_{U-1}] for t >= 1, m the first of the largest of v_{t-1}(2U - 2) (shift 1) and, where skip(2U - 1),
//   v_{t-1}(2U - 3) (shift 2);  q_0 = (U == 1 ? y_0[c_0] : 0)
//   the path is the one of the largest q_t, the earliest t among equals: it enters state 2U - 1 at that step t* and is not defined
//   behind it.  The value is q_{t*}.
// Outputs: *value, and span [WW_CTC_SCORE_MAX_TARGET][2] int8: span[u] = {first step, last step} at which the best path is in state
// 2u + 1 (in prefix mode the last label's pair is {t*, t*}); rows u >= U are -1; value == 0.0f means there is no path - T too short
// for the target, a zero posterior on every path, underflow - and every row is -1.  All 18 bytes are written by every call.
#pragma once

#include "ctc_score.h"

// y: T rows of L values, `ld` values from one row to the next; the arguments are ww_ctc_score_row's.  span: 18 bytes.
WW_CTC_HD inline void ww_ctc_align_row(const float *y, int T, int L, int ld, const int32_t *c, int U, int mode, float *value, int8_t *span) {
  const int blank = L - 1, S = 2 * U + 1;
  float v[2 * WW_CTC_SCORE_MAX_TARGET + 1], b[2 * WW_CTC_SCORE_MAX_TARGET + 1];
  uint8_t bp[WW_CTC_SCORE_MAX_STEPS][2 * WW_CTC_SCORE_MAX_TARGET + 1];
  for (int s = 0; s < S; ++s) v[s] = 0.0f;
  v[0] = y[blank];
  v[1] = y[c[0]];
  float Q = U == 1 ? y[c[0]] : 0.0f;  // the largest q_t so far, first reached at t_star by shift q_shift
  int t_star = 0, q_shift = 0;
  const bool skip_last = ww_cs_skip(c, S - 2);
  for (int t = 1; t < T; ++t) {
    const float *row = y + (long long)t * ld;
    if (mode == WW_CTC_SCORE_PREFIX) {
      float m = v[S - 3];
      int sh = 1;
      if (skip_last && v[S - 4] > m) m = v[S - 4], sh = 2;
      const float q = ww_cs_mul(m, row[c[U - 1]]);
      if (q > Q) Q = q, t_star = t, q_shift = sh;
    }
    for (int s = 0; s < S; ++s) {
      float best = v[s];
      int sh = 0;
      if (s >= 1 && v[s - 1] > best) best = v[s - 1], sh = 1;
      if (ww_cs_skip(c, s) && v[s - 2] > best) best = v[s - 2], sh = 2;
      bp[t][s] = (uint8_t)sh;
      b[s] = ww_cs_mul(best, row[ww_cs_cls(c, s, blank)]);
    }
    for (int s = 0; s < S; ++s) v[s] = b[s];
  }
  for (int j = 0; j < 2 * WW_CTC_SCORE_MAX_TARGET; ++j) span[j] = -1;
  int s, t;  // the back-trace starts in state s at step t
  if (mode == WW_CTC_SCORE_PREFIX) {
    *value = Q;
    if (Q == 0.0f) return;
    span[2 * (U - 1)] = span[2 * (U - 1) + 1] = (int8_t)t_star;
    s = S - 2 - q_shift;
    t = t_star - 1;
  } else {
    s = v[S - 1] > v[S - 2] ? S - 1 : S - 2;
    *value = v[s];
    if (v[s] == 0.0f) return;
    t = T - 1;
  }
  for (; t >= 0; --t) {
    if (s & 1) {
      const int u = (s - 1) >> 1;
      if (span[2 * u + 1] < 0) span[2 * u + 1] = (int8_t)t;
      span[2 * u] = (int8_t)t;
    }
    if (t >= 1) s -= bp[t][s];
  }
}
