// ctc_score.h - the CTC forward algorithm over one window's per-step class posteriors: the probability that the window's label
// sequence reads a target.  The reference trains Arik_CRNN_CTC with K.ctc_batch_cost (wwdetect/CRNN/train.py:184-200) against
// [HEY][SNIPS]; that loss is -log of this quantity, so this is the number those models were optimised to make large on a wake word -
// a score that takes a threshold, where the greedy decode (ctc_decode.h) gives a string to compare.  One definition for
// ctc_score_kernel (ctc_score.hip: the same operations, a lattice state per lane), ww_ctc_score_rows (api.hip: this function over
// host arrays) and the host check (tests/native/ctc_score_check.cpp).  Plain C++ that a device compiler also takes: no HIP header,
// no HIP call.  wwhip/ctc.py: score is the same statement in float64.
//
// y [T][L]: the posteriors, the blank is class L - 1.  A target c[0 .. U), 1 <= U <= WW_CTC_SCORE_MAX_TARGET, labels in [0, L - 2],
// repeats allowed.  States s = 0 .. 2U: an even s is the blank, an odd s is label c[(s - 1) / 2]; cls(s) is that class.
// skip(s): s is odd, s >= 3 and c[(s - 1) / 2] != c[(s - 3) / 2] (between two equal labels the blank cannot be left out).
//   a_0(0) = y_0[blank], a_0(1) = y_0[c_0], every other state 0
//   a_t(s) = ((a_{t-1}(s) + a_{t-1}(s - 1)) + (skip(s) ? a_{t-1}(s - 2) : 0)) * y_t[cls(s)]      t >= 1; a state below 0 is +0
// WW_CTC_SCORE_EXACT - the loss's quantity, P(decode == target):   a_{T-1}(2U) + a_{T-1}(2U - 1)
// WW_CTC_SCORE_PREFIX - the trigger rule's (wwhip/ctc.py: is_wakeword, "starts with"), P(decode starts with target): the paths that
// first complete the target at step t, summed -
//   e_t = (a_{t-1}(2U - 2) + (skip(2U - 1) ? a_{t-1}(2U - 3) : 0)) * y_t[c_{U-1}]                t >= 1
//   P_0 = (U == 1 ? y_0[c_0] : 0),  P_t = P_{t-1} + e_t,  the score is P_{T-1}
// (what follows a completed target is free, and the rows of y sum to 1).  A path is a class per step; "decode" is the collapse of a
// path: repeats merged, blanks dropped.  T < U + (the number of equal neighbours in c) gives exactly 0 in both modes.
//
// Arithmetic: every + and * above is ONE float32 operation rounded once, in the order written, never fused into a multiply-add
// (ww_cs_add / ww_cs_mul below: what __fadd_rn / __fmul_rn promise on a device) - so the kernel, whose lanes do these operations in
// this order, gives this function's bits.  The linear domain with no rescaling, which is why T stops at WW_CTC_SCORE_MAX_STEPS: a
// window's score is a sum of products of T posteriors and a posterior of 0.1 on every step of the best path still leaves 1e-19 at
// T = 19.  Values under FLT_MIN may flush to zero where the hardware is set to do so (neither this host code nor the library's
// kernels ask for it): the accuracy statement against float64 carries an absolute term for it.
//
// It reads the posteriors themselves, as the decode does.  Keras' ctc_batch_cost takes log(y + 1e-7) and tf's ctc_loss then applies
// a softmax to those logarithms again: a renormalisation of every row by sum(y + 1e-7), which the library does not copy.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WW_CTC_HD __host__ __device__
#else
#define WW_CTC_HD
#endif

#define WW_CTC_SCORE_MAX_TARGET 9   // labels in one target
#define WW_CTC_SCORE_MAX_TARGETS 8  // targets in one call
#define WW_CTC_SCORE_MAX_STEPS 64   // T
#define WW_CTC_SCORE_EXACT 0
#define WW_CTC_SCORE_PREFIX 1

// one rounding each, and nothing for a compiler to contract: the pragma takes the licence away inside these two bodies, whatever
// -ffp-contract says (a compiler without it needs -ffp-contract=off)
WW_CTC_HD inline float ww_cs_add(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a + b;
}
WW_CTC_HD inline float ww_cs_mul(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a * b;
}

// the class of state s and whether s - 2 feeds it (0 <= s <= 2U)
WW_CTC_HD inline int ww_cs_cls(const int32_t *c, int s, int blank) { return (s & 1) ? c[(s - 1) >> 1] : blank; }
WW_CTC_HD inline bool ww_cs_skip(const int32_t *c, int s) { return (s & 1) && s >= 3 && c[(s - 1) >> 1] != c[(s - 3) >> 1]; }

// y: T rows of L values, `ld` values from one row to the next.  1 <= T, 2 <= L, 1 <= U <= WW_CTC_SCORE_MAX_TARGET, c[u] in [0, L - 2].
WW_CTC_HD inline float ww_ctc_score_row(const float *y, int T, int L, int ld, const int32_t *c, int U, int mode) {
  const int blank = L - 1, S = 2 * U + 1;
  float a[2 * WW_CTC_SCORE_MAX_TARGET + 1], b[2 * WW_CTC_SCORE_MAX_TARGET + 1];
  for (int s = 0; s < S; ++s) a[s] = 0.0f;
  a[0] = y[blank];
  a[1] = y[c[0]];
  float P = U == 1 ? y[c[0]] : 0.0f;
  const bool skip_last = ww_cs_skip(c, S - 2);
  for (int t = 1; t < T; ++t) {
    const float *row = y + (long long)t * ld;
    if (mode == WW_CTC_SCORE_PREFIX) P = ww_cs_add(P, ww_cs_mul(ww_cs_add(a[S - 3], skip_last ? a[S - 4] : 0.0f), row[c[U - 1]]));
    for (int s = 0; s < S; ++s) {
      const float a1 = s >= 1 ? a[s - 1] : 0.0f, a2 = ww_cs_skip(c, s) ? a[s - 2] : 0.0f;
      b[s] = ww_cs_mul(ww_cs_add(ww_cs_add(a[s], a1), a2), row[ww_cs_cls(c, s, blank)]);
    }
    for (int s = 0; s < S; ++s) a[s] = b[s];
  }
  return mode == WW_CTC_SCORE_PREFIX ? P : ww_cs_add(a[S - 1], a[S - 2]);
}

#include <cstdio>
// (host code: a device compiler parses it and emits nothing for it)
// What every entry point of the family refuses (include/wwhip.h: ww_ctc_score_*), the rule named in `why`; true = acceptable.
// targets [K][WW_CTC_SCORE_MAX_TARGET], target_lens [K].
inline bool ww_ctc_score_args_ok(int T, int L, const int32_t *targets, const int32_t *target_lens, int K, int mode, char *why, size_t n_why) {
  if (T < 1 || T > WW_CTC_SCORE_MAX_STEPS) return snprintf(why, n_why, "T = %d outside 1..%d (the linear domain is not rescaled)", T, WW_CTC_SCORE_MAX_STEPS), false;
  if (L < 2 || L > 64) return snprintf(why, n_why, "L = %d outside 2..64", L), false;
  if (K < 1 || K > WW_CTC_SCORE_MAX_TARGETS) return snprintf(why, n_why, "K = %d targets outside 1..%d", K, WW_CTC_SCORE_MAX_TARGETS), false;
  if (mode != WW_CTC_SCORE_EXACT && mode != WW_CTC_SCORE_PREFIX) return snprintf(why, n_why, "unknown mode %d (WW_CTC_SCORE_EXACT, WW_CTC_SCORE_PREFIX)", mode), false;
  if (!targets || !target_lens) return snprintf(why, n_why, "targets / target_lens are NULL"), false;
  for (int k = 0; k < K; ++k) {
    const int U = target_lens[k];
    if (U < 1 || U > WW_CTC_SCORE_MAX_TARGET) return snprintf(why, n_why, "target %d has U = %d labels, outside 1..%d", k, U, WW_CTC_SCORE_MAX_TARGET), false;
    for (int u = 0; u < U; ++u) {
      const int c = targets[k * WW_CTC_SCORE_MAX_TARGET + u];
      if (c < 0 || c > L - 2) return snprintf(why, n_why, "target %d label %d is %d, outside [0, L - 2] = [0, %d] (the blank is class L - 1)", k, u, c, L - 2), false;
    }
  }
  return true;
}
