// ctc_decode.h - the greedy CTC decode of one sequence of per-step class posteriors: what K.ctc_decode(greedy=True) does to a row of
// wwdetect/CRNN/evaluate.py:100-150 (eval_CTC).  One definition for gru_tail_ctc_kernel (crnn.hip: the 19 rows in LDS),
// ctc_greedy_kernel (crnn.hip: any [n][T][L] in global memory) and the host check (tests/native/ctc_decode_check.cpp).
// Plain C++ that a device compiler also takes: no HIP header, no HIP call.
//
// Per step the argmax over the L classes, the LOWEST index on a tie; the class is emitted when it is not the blank (class L - 1) and
// differs from the previous step's argmax.  The blank counts as a previous value: a, blank, a reads "a a"; a, a reads "a".
// wwhip/ctc.py: greedy_decode is the same statement in numpy.
//
// Keras' ctc_decode takes log(y + 1e-7) of the posteriors before its argmax.  That map is monotone, so it cannot reverse an order;
// it can only turn a strict order of two float32 posteriors into a tie where both round to the same logarithm.  This function
// decodes the posteriors themselves, as they are stored.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WW_CTC_HD __host__ __device__
#else
#define WW_CTC_HD
#endif

// steps: T rows of L values, `ld` values from one row to the next.  labels[0 .. max_labels): the first decoded labels, the rest -1.
// Returns the whole decoded length (it may exceed max_labels).  T >= 0, L >= 1, max_labels >= 0.
WW_CTC_HD inline int32_t ww_ctc_greedy_row(const float *steps, int T, int L, int ld, int32_t *labels, int max_labels) {
  const int blank = L - 1;
  int prev = -1, n = 0;
  for (int t = 0; t < T; ++t) {
    const float *row = steps + (long long)t * ld;
    int best = 0;
    float bv = row[0];
    for (int c = 1; c < L; ++c) {
      const float v = row[c];
      if (v > bv) {  // (strictly: a tie keeps the lower index)
        bv = v;
        best = c;
      }
    }
    if (best != blank && best != prev) {
      if (n < max_labels) labels[n] = best;
      ++n;
    }
    prev = best;
  }
  for (int k = n; k < max_labels; ++k) labels[k] = -1;
  return n;
}
