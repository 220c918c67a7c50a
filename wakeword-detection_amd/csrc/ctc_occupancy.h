// ctc_occupancy.h - the forward-backward occupancy of a target over one window's per-step class posteriors: GIVEN that the window
// reads the target, how much of each step belongs to each label, summed over all the paths that read it and not only the best one.
// It is the soft counterpart of ctc_align.h's span (one best path gives a span quantised to a conv step and no confidence; this
// says how sure the model is of a boundary), in prefix mode the distribution of the step at which the wake word was completed,
// and the missing half of the quantity the reference trains Arik_CRNN_CTC with: K.ctc_batch_cost (wwdetect/CRNN/train.py:184-200)
// is -log of ctc_score.h's exact score, and its gradient with respect to the logits of step t is y_t[c] minus the class occupancy
// cls[t][c] below.  One definition for ctc_occupancy_kernel (ctc_occupancy.hip: the same operations, a lattice state per lane),
// ww_ctc_occupancy_rows (api.hip: this function over host arrays) and the host check (tests/native/ctc_occupancy_check.cpp).  Plain
// C++ that a device compiler also takes: no HIP header, no HIP call.  wwhip/ctc.py: occupancy is the same statement in float64.
//
// y [T][L], the blank L - 1, the target c[0 .. U), the states s = 0 .. 2U, cls(s) and skip(s): ctc_score.h's, and so are the limits
// and the argument rule (ww_ctc_score_args_ok).  a_t(s) is that header's forward recurrence, the same operations in the same
// order, and the value returned carries the bits of ww_ctc_score_row.
//
// WW_CTC_SCORE_EXACT.  The backward variable does NOT contain y_t, so nothing is ever divided by a posterior:
//   b_{T-1}(2U) = b_{T-1}(2U - 1) = 1, every other state 0
//   m_{t+1}(s) = b_{t+1}(s) * y_{t+1}[cls(s)]
//   b_t(s)     = (m_{t+1}(s) + m_{t+1}(s + 1)) + (skip(s + 2) ? m_{t+1}(s + 2) : 0)          a state above 2U is +0
//   Z          = a_{T-1}(2U) + a_{T-1}(2U - 1)                                               the score
//   g_t(s)     = (a_t(s) * b_t(s)) / Z
//   occ[t][u]  = g_t(2u + 1)
//   cls[t][k]  = the sum of g_t(s) over the states with cls(s) == k, added in ascending s, starting from the first such state (not
//                from 0); a class with no state is +0
// For every t the g_t(s) sum to 1 over s, so a row of cls sums to 1 and 1 - sum_u occ[t][u] is the blank's share.
//
// WW_CTC_SCORE_PREFIX.  The live states are 0 .. 2U - 2; e_t is ctc_score.h's completion term,
//   e_t = (a_{t-1}(2U - 2) + (skip(2U - 1) ? a_{t-1}(2U - 3) : 0)) * y_t[c_{U-1}]  for t >= 1,  e_0 = (U == 1 ? y_0[c_0] : 0)
//   Z = P_{T-1} = ((e_0 + e_1) + e_2) + ...                                                  the score
//   b_{T-1}(s) = 0;  b_t(s) for s <= 2U - 2 is the three-term sum above with m_{t+1}(2U - 1) replaced by y_{t+1}[c_{U-1}] and the
//   states above 2U - 1 absent: what follows completion is free, so its backward value is 1
//   occ[t][u]     = (a_t(2u + 1) * b_t(2u + 1)) / Z    for u < U - 1
//   occ[t][U - 1] = e_t / Z                            the posterior of the completion step: it sums to 1 over t
// There is no cls in this mode (the steps behind the completion belong to no class of the target): passing one is refused.
// (The function below pins b_t(2U - 1) = 1 and b_t(2U) = 0 at every t and keeps e_t where a_t(2U - 1) would sit: 1 * y and e * 1
// are exact, so one loop serves both modes with the operations above and no other.)
//
// Z == 0 (T too short for the target, a zero posterior on every path, underflow): the value is 0 and every occ / cls entry is +0.
// Rows u >= U of occ are +0.  Every byte of occ [T][WW_CTC_SCORE_MAX_TARGET] and of cls [T][L] is written by every call.
//
// Arithmetic: every +, * and the one / above is ONE float32 operation rounded once, in the order written, never contracted
// (ww_cs_add / ww_cs_mul of ctc_score.h and ww_cs_div below: what __fadd_rn / __fmul_rn / __fdiv_rn promise on a device).  The
// linear domain with no rescaling, T <= WW_CTC_SCORE_MAX_STEPS, as for the score; a_t(s) b_t(s) is the probability of the paths
// through state s at step t, a part of Z, so g never exceeds 1 by more than its roundings.  Against the float64 statement on the
// same float32 posteriors: a_t(s) carries 3 roundings a step (3t), b_t(s) 3 a step (3 (T - 1 - t)), Z 3 (T - 1) + 1, the product 1
// and the division 1 - |g32 - g64| <= (6 T + 4) 2^-24 g64 to first order, 2U more for a cls entry's additions, plus an absolute
// term for what flushes or rounds under FLT_MIN (tests/ctc_occupancy64.py derives both).
#pragma once

#include "ctc_score.h"

WW_CTC_HD inline float ww_cs_div(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a / b;
}

// y: T rows of L values, `ld` values from one row to the next; the arguments are ww_ctc_score_row's.  occ: T rows of
// WW_CTC_SCORE_MAX_TARGET values; cls: T rows of L values, or NULL (it must be NULL in prefix mode).  Returns Z.
WW_CTC_HD inline float ww_ctc_occupancy_row(const float *y, int T, int L, int ld, const int32_t *c, int U, int mode, float *occ, float *cls) {
  const int blank = L - 1, S = 2 * U + 1;
  const bool prefix = mode == WW_CTC_SCORE_PREFIX;
  float a[WW_CTC_SCORE_MAX_STEPS][2 * WW_CTC_SCORE_MAX_TARGET + 1];  // a_t(s); in prefix mode e_t where a_t(2U - 1) would sit
  float b[2 * WW_CTC_SCORE_MAX_TARGET + 1], m[2 * WW_CTC_SCORE_MAX_TARGET + 3], g[2 * WW_CTC_SCORE_MAX_TARGET + 1];
  for (int s = 0; s < S; ++s) a[0][s] = 0.0f;
  a[0][0] = y[blank];
  a[0][1] = y[c[0]];
  float P = U == 1 ? y[c[0]] : 0.0f;
  const bool skip_last = ww_cs_skip(c, S - 2);
  for (int t = 1; t < T; ++t) {
    const float *row = y + (long long)t * ld, *p = a[t - 1];
    for (int s = 0; s < S; ++s) {
      const float a1 = s >= 1 ? p[s - 1] : 0.0f, a2 = ww_cs_skip(c, s) ? p[s - 2] : 0.0f;
      a[t][s] = ww_cs_mul(ww_cs_add(ww_cs_add(p[s], a1), a2), row[ww_cs_cls(c, s, blank)]);
    }
    if (prefix) P = ww_cs_add(P, ww_cs_mul(ww_cs_add(p[S - 3], skip_last ? p[S - 4] : 0.0f), row[c[U - 1]]));
  }
  const float Z = prefix ? P : ww_cs_add(a[T - 1][S - 1], a[T - 1][S - 2]);
  if (prefix) {  // e_t = (a_{t-1}(2U - 2) + a_{t-1}(2U - 3) or 0) * y_t[c_{U-1}], the term P took at step t; a_t(2U - 1) is not live
    for (int t = T - 1; t >= 1; --t)
      a[t][S - 2] = ww_cs_mul(ww_cs_add(a[t - 1][S - 3], skip_last ? a[t - 1][S - 4] : 0.0f), y[(long long)t * ld + c[U - 1]]);
    a[0][S - 2] = U == 1 ? y[c[0]] : 0.0f;
  }
  for (int s = 0; s < S; ++s) b[s] = 0.0f;
  b[S - 2] = 1.0f;
  b[S - 1] = prefix ? 0.0f : 1.0f;
  for (int t = T - 1; t >= 0; --t) {
    float *o = occ + (long long)t * WW_CTC_SCORE_MAX_TARGET;
    for (int s = 0; s < S; ++s) g[s] = Z == 0.0f ? 0.0f : ww_cs_div(ww_cs_mul(a[t][s], b[s]), Z);
    for (int u = 0; u < WW_CTC_SCORE_MAX_TARGET; ++u) o[u] = u < U ? g[2 * u + 1] : 0.0f;
    if (cls) {
      for (int k = 0; k < L; ++k) {
        float acc = 0.0f;
        bool have = false;
        for (int s = 0; s < S; ++s)
          if (ww_cs_cls(c, s, blank) == k) acc = have ? ww_cs_add(acc, g[s]) : g[s], have = true;
        cls[(long long)t * L + k] = acc;
      }
    }
    if (t == 0) break;
    const float *row = y + (long long)t * ld;
    for (int s = 0; s < S; ++s) m[s] = ww_cs_mul(b[s], row[ww_cs_cls(c, s, blank)]);
    m[S] = m[S + 1] = 0.0f;
    for (int s = 0; s < S; ++s) b[s] = ww_cs_add(ww_cs_add(m[s], m[s + 1]), (s + 2 < S && ww_cs_skip(c, s + 2)) ? m[s + 2] : 0.0f);
    if (prefix) b[S - 2] = 1.0f, b[S - 1] = 0.0f;
  }
  return Z;
}

// What every entry point of the family refuses (include/wwhip.h: ww_ctc_occupancy_*): ww_ctc_score_args_ok's rules, a NULL value or
// occ, and a cls in prefix mode; the rule named in `why`; true = acceptable.
inline bool ww_ctc_occupancy_args_ok(int T, int L, const int32_t *targets, const int32_t *target_lens, int K, int mode, const void *value,
                                     const void *occ, const void *cls, char *why, size_t n_why) {
  if (!ww_ctc_score_args_ok(T, L, targets, target_lens, K, mode, why, n_why)) return false;
  if (!value || !occ) return snprintf(why, n_why, "value / occ are NULL"), false;
  if (cls && mode == WW_CTC_SCORE_PREFIX) return snprintf(why, n_why, "cls with WW_CTC_SCORE_PREFIX (the class occupancy is defined in exact mode only)"), false;
  return true;
}
