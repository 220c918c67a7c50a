// ctc_beam.h - CTC prefix beam search over one window's per-step class posteriors: the P most probable LABEL STRINGS and their
// probabilities, where the greedy decode (ctc_decode.h) collapses the most probable PATH and ctc_score.h needs its targets named in
// advance.  What K.ctc_decode(greedy=False, beam_width, top_paths) is asked for.  One definition for ctc_beam_kernel (ctc_beam.hip:
// the same operations, a beam slot per lane), ww_ctc_beam_rows (api.hip: ww_ctc_beam_row over host arrays) and the host check
// (tests/native/ctc_beam_check.cpp).  Plain C++ that a device compiler also takes: no HIP header, no HIP call.  wwhip/ctc.py:
// beam_search is the same statement in float64.
//
// y [T][L]: the posteriors, the blank is class L - 1.  1 <= T <= WW_CTC_BEAM_MAX_T, 2 <= L <= 8, beam width 1 <= W <=
// WW_CTC_BEAM_MAX_WIDTH, 1 <= P <= min(W, WW_CTC_BEAM_MAX_PATHS) reported paths, 1 <= max_labels <= T.
//
// The key.  A prefix (a label string) is one 64-bit key: its length in bits 57..61, its labels below at 3 bits each, the first label
// in bits 54..56 - so ascending key order is shorter first, then lexicographic (ww_cb_* below; the packing is static_assert'ed).
//
// The beam: at most W entries (key, pb, pnb) - pb the probability of the paths that collapse to the prefix and end in the blank, pnb
// of those that end in its last label.  It starts as the empty prefix with (1, 0).  Step t takes row y_t; for every entry A, with
// tot = pb + pnb:
//   stay     pb' = tot * y[blank];  pnb' = pnb * y[last(A)], which is 0 for the empty prefix
//   extend   for every label c in 0 .. L - 2:  ext = (c == last(A) ? pb : tot) * y[c]
//            A + c is itself a beam entry B:  pnb'(B) = pnb(B) * y[c] + ext   (B's stay term first, then ONE addition; B has exactly
//                                             one parent, so nothing else is ever added to it)
//            otherwise:                       A + c is a new candidate (0, ext)
// A candidate's total is pb' + pnb'.  The next beam is the first W candidates in the order: total descending, then key ascending,
// where a NaN total ranks as -1 and +Inf as the number it is (ww_cb_rank, ww_cb_before: a total order, keys being distinct - any
// correct selection gives the same beam).  Only these are candidates: a beam that is not full has no empty slots competing, and a
// candidate of probability 0 (a a a in two steps) is an ordinary one.  After step T - 1 the first P entries in the same order are
// reported: labels (the first max_labels of them, padded with -1), the whole length, prob = pb + pnb.  A reported path whose
// probability is 0 - or a place the beam has no entry for - is absent: length -1, every label -1, prob 0.
//
// Arithmetic: every + and * above is ONE float32 operation rounded once, in the order written, never fused (ww_cs_add / ww_cs_mul of
// ctc_score.h), so the kernel, whose lanes do these operations and these comparisons, gives this function's bits.  The linear domain
// with no rescaling, as the score: T stops at 19.
//
// Accuracy, against the float64 statement on the same float32 posteriors WITH THE SAME PRUNING DECISIONS (the same beam after every
// step), as ctc_score.h derives its (3T + 2) 2^-24.  Every quantity is a sum of products of non-negative numbers, so relative errors
// do not amplify: a sum or product of terms each within (1 + u)^k of its exact value, rounded once, is within (1 + u)^(k + 1),
// u = 2^-24.  Write d_t for the largest exponent k over the pb and pnb of step t.  d_{-1} = 0 (1 and 0 are exact).  One step:
// tot costs one rounding (d + 1), pb' = tot * y one more (d + 2); pnb * y is d + 1, ext = (pb or tot) * y is at most d + 2, and
// their one addition d + 3.  So d_t <= d_{t-1} + 3, d_{T-1} <= 3T, and the reported pb + pnb is within (1 + u)^(3T + 1), which is
// at most 1 + (3T + 2) u for every T here (the second-order term (3T + 1)^2 u^2 / 2 is under 2e-4 u at T = 19):
//     relative error <= (3T + 2) 2^-24                                                       (WW_CTC_BEAM_REL_ULPS(T) units of 2^-24)
// Flushing: values under FLT_MIN may be flushed to zero where the hardware is set so (neither this host code nor the kernel ask for
// it).  Each flushed result moves a value by less than 2^-126, and it travels on multiplied by posteriors <= 1.  A reported
// prefix depends on the prefixes of its ancestor chain only (at most T + 1 of them), each with five operations per step, so the
// absolute term is 5 T (T + 1) 2^-126.
//
// Parity.  This is the textbook prefix search (Graves; Hannun et al. 2014, without a language model) on the posteriors themselves.
// It is NOT a bit copy of TensorFlow's decoder behind K.ctc_decode, which works on log(y + 1e-7) in the log domain, merges with
// log-sum-exp and is not installed where this library is tested: the parity target is the float64 statement, as the resampler's is
// its float64 statement and not librosa's bits.
#pragma once

#include <cstdint>

#include "ctc_score.h"

#define WW_CTC_BEAM_MAX_T 19      // steps, and so labels in a prefix
#define WW_CTC_BEAM_MAX_L 8       // classes with the blank: a label fits 3 bits
#define WW_CTC_BEAM_MAX_WIDTH 64  // W: a beam slot per lane of a wave
#define WW_CTC_BEAM_MAX_PATHS 8   // P
#define WW_CTC_BEAM_REL_ULPS(T) (3 * (T) + 2)

#define WW_CB_LABEL_BITS 3
#define WW_CB_LEN_SHIFT (WW_CB_LABEL_BITS * WW_CTC_BEAM_MAX_T)  // 57
#define WW_CB_LEN_BITS 5
static_assert(WW_CTC_BEAM_MAX_L - 2 < (1 << WW_CB_LABEL_BITS), "a label (0 .. L - 2) fits its field");
static_assert(WW_CTC_BEAM_MAX_T < (1 << WW_CB_LEN_BITS), "a length (0 .. T) fits its field");
static_assert(WW_CB_LEN_SHIFT + WW_CB_LEN_BITS <= 64, "length and labels fit one 64-bit key");
static_assert(WW_CTC_BEAM_MAX_WIDTH == 64, "ctc_beam_kernel keeps a beam slot per lane of a 64-wide wave");
#define WW_CB_NO_KEY (~(uint64_t)0)  // no prefix has it (a length field of 31)

WW_CTC_HD inline int ww_cb_len(uint64_t key) { return (int)(key >> WW_CB_LEN_SHIFT); }
// label i of a prefix, 0 <= i < len
WW_CTC_HD inline int ww_cb_label(uint64_t key, int i) { return (int)(key >> (WW_CB_LEN_SHIFT - WW_CB_LABEL_BITS * (i + 1))) & ((1 << WW_CB_LABEL_BITS) - 1); }
// the last label, -1 for the empty prefix
WW_CTC_HD inline int ww_cb_last(uint64_t key) {
  const int n = ww_cb_len(key);
  return n ? ww_cb_label(key, n - 1) : -1;
}
// A + c (len(A) < WW_CTC_BEAM_MAX_T)
WW_CTC_HD inline uint64_t ww_cb_append(uint64_t key, int c) {
  const int n = ww_cb_len(key);
  return key + ((uint64_t)1 << WW_CB_LEN_SHIFT) + ((uint64_t)c << (WW_CB_LEN_SHIFT - WW_CB_LABEL_BITS * (n + 1)));
}
// A without its last label (len(A) >= 1)
WW_CTC_HD inline uint64_t ww_cb_parent(uint64_t key) {
  const int n = ww_cb_len(key), sh = WW_CB_LEN_SHIFT - WW_CB_LABEL_BITS * n;
  return (key - ((uint64_t)1 << WW_CB_LEN_SHIFT)) & ~((uint64_t)((1 << WW_CB_LABEL_BITS) - 1) << sh);
}

// the step's operations, one rounding each
WW_CTC_HD inline float ww_cb_tot(float pb, float pnb) { return ww_cs_add(pb, pnb); }
WW_CTC_HD inline float ww_cb_stay_pb(float tot, float y_blank) { return ww_cs_mul(tot, y_blank); }
// y_last: y[last(A)]; whatever it is for the empty prefix (last < 0), the result is 0
WW_CTC_HD inline float ww_cb_stay_pnb(float pnb, int last, float y_last) { return last < 0 ? 0.0f : ww_cs_mul(pnb, y_last); }
WW_CTC_HD inline float ww_cb_ext(float pb, float tot, int last, int c, float y_c) { return ww_cs_mul(c == last ? pb : tot, y_c); }
WW_CTC_HD inline float ww_cb_merge(float stay_pnb, float ext) { return ww_cs_add(stay_pnb, ext); }
// the order: rank descending, then key ascending
WW_CTC_HD inline float ww_cb_rank(float total) { return total != total ? -1.0f : total; }
WW_CTC_HD inline bool ww_cb_before(float rank_a, uint64_t key_a, float rank_b, uint64_t key_b) {
  return rank_a > rank_b || (rank_a == rank_b && key_a < key_b);
}
// what place p of the report holds: the entry (p < nb) or nothing.  labels [max_labels]
WW_CTC_HD inline void ww_cb_report(bool have, uint64_t key, float pb, float pnb, int max_labels, int32_t *labels, int32_t *length, float *prob) {
  const float pr = have ? ww_cb_tot(pb, pnb) : 0.0f;
  const bool absent = !have || pr == 0.0f;
  const int n = absent ? -1 : ww_cb_len(key);
  for (int i = 0; i < max_labels; ++i) labels[i] = i < n ? ww_cb_label(key, i) : -1;
  *length = n;
  *prob = absent ? 0.0f : pr;
}

// (host code from here on: a device compiler parses it and emits nothing for it)
// y: T rows of L values, `ld` values from one row to the next; the arguments have passed ww_ctc_beam_args_ok.
// labels [P][max_labels], lengths [P], prob [P].
inline void ww_ctc_beam_row(const float *y, int T, int L, int ld, int W, int P, int max_labels, int32_t *labels, int32_t *lengths, float *prob) {
  constexpr int MW = WW_CTC_BEAM_MAX_WIDTH;
  const int blank = L - 1;
  uint64_t key[MW], skey[MW];
  float pb[MW], pnb[MW], tot[MW], st_pb[MW], st_pnb[MW], spb[MW], spnb[MW], srank[MW];
  uint8_t claimed[MW];
  int nb = 1, ns = 0;
  key[0] = 0;
  pb[0] = 1.0f;
  pnb[0] = 0.0f;
  // a candidate into the first-W list, which is kept in the order
  auto offer = [&](uint64_t k, float cpb, float cpnb) {
    const float r = ww_cb_rank(ww_cb_tot(cpb, cpnb));
    if (ns == W && !ww_cb_before(r, k, srank[W - 1], skey[W - 1])) return;
    int i = ns < W ? ns++ : W - 1;
    for (; i > 0 && ww_cb_before(r, k, srank[i - 1], skey[i - 1]); --i) {
      skey[i] = skey[i - 1]; spb[i] = spb[i - 1]; spnb[i] = spnb[i - 1]; srank[i] = srank[i - 1];
    }
    skey[i] = k; spb[i] = cpb; spnb[i] = cpnb; srank[i] = r;
  };
  for (int t = 0; t < T; ++t) {
    const float *row = y + (long long)t * ld;
    for (int j = 0; j < nb; ++j) {
      const int last = ww_cb_last(key[j]);
      tot[j] = ww_cb_tot(pb[j], pnb[j]);
      st_pb[j] = ww_cb_stay_pb(tot[j], row[blank]);
      st_pnb[j] = ww_cb_stay_pnb(pnb[j], last, last < 0 ? 0.0f : row[last]);
      claimed[j] = 0;
    }
    // an entry whose parent is in the beam takes that parent's extension
    for (int j = 0; j < nb; ++j) {
      if (!ww_cb_len(key[j])) continue;
      const uint64_t pk = ww_cb_parent(key[j]);
      for (int p = 0; p < nb; ++p)
        if (key[p] == pk) {
          const int c = ww_cb_last(key[j]);
          st_pnb[j] = ww_cb_merge(st_pnb[j], ww_cb_ext(pb[p], tot[p], ww_cb_last(pk), c, row[c]));
          claimed[p] |= (uint8_t)(1u << c);
          break;
        }
    }
    ns = 0;
    for (int j = 0; j < nb; ++j) {
      offer(key[j], st_pb[j], st_pnb[j]);
      const int last = ww_cb_last(key[j]);
      for (int c = 0; c < blank; ++c)
        if (!((claimed[j] >> c) & 1)) offer(ww_cb_append(key[j], c), 0.0f, ww_cb_ext(pb[j], tot[j], last, c, row[c]));
    }
    nb = ns;
    for (int j = 0; j < nb; ++j) {
      key[j] = skey[j]; pb[j] = spb[j]; pnb[j] = spnb[j];
    }
  }
  for (int p = 0; p < P; ++p) ww_cb_report(p < nb, p < nb ? key[p] : 0, p < nb ? pb[p] : 0.0f, p < nb ? pnb[p] : 0.0f, max_labels, labels + (long long)p * max_labels, lengths + p, prob + p);
}

// What every entry point of the family refuses (include/wwhip.h: ww_ctc_beam_*), the rule named in `why`; true = acceptable.
inline bool ww_ctc_beam_args_ok(int T, int L, int W, int P, int max_labels, char *why, size_t n_why) {
  if (T < 1 || T > WW_CTC_BEAM_MAX_T) return snprintf(why, n_why, "T = %d outside 1..%d (a prefix is one 64-bit key; the linear domain is not rescaled)", T, WW_CTC_BEAM_MAX_T), false;
  if (L < 2 || L > WW_CTC_BEAM_MAX_L) return snprintf(why, n_why, "L = %d outside 2..%d", L, WW_CTC_BEAM_MAX_L), false;
  if (W < 1 || W > WW_CTC_BEAM_MAX_WIDTH) return snprintf(why, n_why, "beam_width = %d outside 1..%d", W, WW_CTC_BEAM_MAX_WIDTH), false;
  const int pmax = W < WW_CTC_BEAM_MAX_PATHS ? W : WW_CTC_BEAM_MAX_PATHS;
  if (P < 1 || P > pmax) return snprintf(why, n_why, "top_paths = %d outside 1..min(beam_width, %d) = 1..%d", P, WW_CTC_BEAM_MAX_PATHS, pmax), false;
  if (max_labels < 1 || max_labels > T) return snprintf(why, n_why, "max_labels = %d outside 1..T = 1..%d", max_labels, T), false;
  return true;
}
