// stream_ctc.h - what a CTC stream bank (include/wwhip.h: ww_stream_create_ctc) adds to a stream bank's tick: the 32-bit word a
// streamed window's decode travels in, the host's unpacking of a tick's words, and the wake-word rule on decoded labels.  Plain C++
// that a device compiler also takes (no HIP header, no HIP call), in the style of ctc_decode.h: crnn.hip packs on the device,
// streams.hip unpacks and runs the rule, tests/native/stream_ctc_check.cpp compiles the file alone under Address + UB sanitizer.
//
// The word.  A window's greedy decode (ctc_decode.h) is a string of labels, each < L - 1 <= 7, of a length 0..19.  One 32-bit word
// holds the WHOLE length in bits 27..31 and label i in bits 3 i .. 3 i + 2 for i < WW_STREAM_CTC_MAX_LABELS = 9 (27 bits); label bits
// past the string's end are zero.  In the polled forms of the tick the word is the value half of the window's {value, tick number}
// tag (common.h: ww_tick_tag; tick_tag_store's `unsigned` overload - the bits never pass through a float), in the waited forms a
// row of the bank's page-locked output block.
//
// The posteriors of a WW_STREAM_CTC_STEPS bank ([2 S][19][L], page-locked) are ordinary stores of the same kernel.  NO order is
// built between those stores and the tag: a tag that has arrived says nothing about the posteriors, which is why such a bank always
// waits for the stream with hipStreamSynchronize and never polls.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WW_SC_HD __host__ __device__
#else
#define WW_SC_HD
#endif

#ifndef WW_STREAM_CTC_MAX_LABELS
#define WW_STREAM_CTC_MAX_LABELS 9  // (include/wwhip.h states it too)
#endif
#define WW_SC_STEPS 19         // rows of posteriors per window = the greatest decoded length
#define WW_SC_LENGTH_SHIFT 27

// labels[0 .. min(length, 9)): each 0..7; length 0..19 (the whole decoded length, as ww_ctc_greedy_row returns it)
WW_SC_HD inline uint32_t ww_sc_pack(const int32_t *labels, int32_t length) {
  uint32_t w = (uint32_t)length << WW_SC_LENGTH_SHIFT;
  const int n = length < WW_STREAM_CTC_MAX_LABELS ? length : WW_STREAM_CTC_MAX_LABELS;
  for (int i = 0; i < n; ++i) w |= ((uint32_t)labels[i] & 7u) << (3 * i);
  return w;
}

// The word's first max_labels labels (1..9), the rest -1 - the row ww_ctc_greedy_row writes for that max_labels.  Returns the length.
WW_SC_HD inline int32_t ww_sc_unpack(uint32_t w, int32_t *labels, int max_labels) {
  const int32_t length = (int32_t)(w >> WW_SC_LENGTH_SHIFT);
  for (int i = 0; i < max_labels; ++i) labels[i] = i < length ? (int32_t)((w >> (3 * i)) & 7u) : -1;
  return length;
}

// ---- host only ----------------------------------------------------------------------------------------------------------------------
// A tick's words where the caller reads them: labels [S][2][max_labels], lengths [S][2]; entries at or past n_post[s] are left as they
// were.  fetch(slot) is the word that arrived in `slot`: 2 s + k, or in the table form (one descriptor per window, in (s, k) order:
// stream_all.h, SA_TABLE) the running window index.
template <typename Fetch>
static inline void sc_scatter(bool table_form, int S, const int32_t *n_post, Fetch &&fetch, int max_labels, int32_t *labels, int32_t *lengths) {
  int w = 0;
  for (int s = 0; s < S; ++s)
    for (int k = 0; k < n_post[s]; ++k, ++w)
      lengths[(size_t)s * 2 + k] = ww_sc_unpack(fetch(table_form ? w : 2 * s + k), labels + ((size_t)s * 2 + k) * max_labels, max_labels);
}

// Does a decode start with target[0 .. n_target)?  wwhip.ctc.is_wakeword's rule (wwdetect/CRNN/evaluate.py:100-150: decoded[:, :2]
// against [HEY][SNIPS]): the whole length reaches n_target and the first n_target labels equal it.  1 <= n_target <= max_labels.
static inline bool sc_starts_with(const int32_t *labels, int32_t length, const int32_t *target, int n_target) {
  if (length < n_target) return false;
  for (int i = 0; i < n_target; ++i)
    if (labels[i] != target[i]) return false;
  return true;
}

// The wake-word stage over a tick's decodes: stream_all.h's sa_trigger_update with the label rule in place of the threshold - the
// same VAD-edge bookkeeping (spokestack/wakeword/tflite.py:134-146), the same fired and fall lists.
//   labels [S][2][max_labels], lengths [S][2], n_post [S] (0..2 windows of the tick)
//   - a stream that is not active FIRES on the first window of the tick whose decode starts with the target: is_active[s] = 1,
//     fired_ids gets s; a stream that is already active does not fire again
//   - fall_ids: the streams whose VAD bit fell (the caller resets them)
// Arguments are the caller's to check (sc_check_trigger).
static inline void sc_trigger_update(int S, const uint8_t *is_speech, uint8_t *is_active, const int32_t *labels, const int32_t *lengths,
                                     const int32_t *n_post, int max_labels, const int32_t *target, int n_target, uint8_t *was_speech,
                                     int32_t *fired_ids, int32_t *n_fired, int32_t *fall_ids, int32_t *n_fall) {
  int nf = 0, nl = 0;
  for (int s = 0; s < S; ++s) {
    const uint8_t sp = is_speech[s] != 0;
    const bool fall = was_speech[s] && !sp;
    was_speech[s] = sp;
    bool hit = false;
    for (int k = 0; k < n_post[s] && !hit; ++k)
      hit = sc_starts_with(labels + ((size_t)s * 2 + k) * max_labels, lengths[(size_t)s * 2 + k], target, n_target);
    if (hit && !is_active[s]) {
      is_active[s] = 1;
      fired_ids[nf++] = s;
    }
    if (fall) fall_ids[nl++] = s;
  }
  *n_fired = nf;
  *n_fall = nl;
}

// The arguments of ww_ctc_trigger_bank_step (include/wwhip.h): 0, or -1 with nothing touched
static inline int sc_check_trigger(int64_t S, const void *is_speech, const void *is_active, const void *labels, const void *lengths,
                                   const int32_t *n_post, int64_t max_labels, const int32_t *target, int64_t n_target, const void *was_speech,
                                   const void *fired_ids, const void *n_fired, const void *fall_ids, const void *n_fall) {
  if (S < 0 || !n_fired || !n_fall || !target) return -1;
  if (max_labels < 1 || max_labels > WW_STREAM_CTC_MAX_LABELS || n_target < 1 || n_target > max_labels) return -1;
  if (S > 0 && (!is_speech || !is_active || !labels || !lengths || !n_post || !was_speech || !fired_ids || !fall_ids)) return -1;
  for (int64_t s = 0; s < S; ++s)
    if (n_post[s] < 0 || n_post[s] > 2) return -1;
  return 0;
}

// The same stage with the SCORE rule (ctc_score.h: a window's forward-algorithm scores for K targets, one per slot): the VAD-edge
// bookkeeping above, and stream_all.h's comparison (sa_trigger_update: the float32 value against a Python float, (double)p > t).
//   scores [S][2][K] (window k of the tick, slot j), n_post [S], thresholds [K]
//   - a stream that is not active FIRES on the first window of the tick on which some slot j has (double)score > thresholds[j]:
//     is_active[s] = 1, fired_ids gets s and fired_slot the exceeding slot with the greatest score on that window, the lowest slot
//     among equals; a stream that is already active does not fire again
//   - fall_ids: the streams whose VAD bit fell (the caller resets them)
// fired_slot may be nullptr.  Arguments are the caller's to check (sc_check_score_trigger).
static inline void sc_score_trigger_update(int S, int K, const uint8_t *is_speech, uint8_t *is_active, const float *scores, const int32_t *n_post,
                                           const double *thresholds, uint8_t *was_speech, int32_t *fired_ids, int32_t *fired_slot,
                                           int32_t *n_fired, int32_t *fall_ids, int32_t *n_fall) {
  int nf = 0, nl = 0;
  for (int s = 0; s < S; ++s) {
    const uint8_t sp = is_speech[s] != 0;
    const bool fall = was_speech[s] && !sp;
    was_speech[s] = sp;
    int win = -1;
    for (int k = 0; k < n_post[s] && win < 0; ++k) {
      const float *p = scores + ((size_t)s * 2 + k) * K;
      for (int j = 0; j < K; ++j)
        if ((double)p[j] > thresholds[j] && (win < 0 || p[j] > p[win])) win = j;
    }
    if (win >= 0 && !is_active[s]) {
      is_active[s] = 1;
      fired_ids[nf] = s;
      if (fired_slot) fired_slot[nf] = win;
      ++nf;
    }
    if (fall) fall_ids[nl++] = s;
  }
  *n_fired = nf;
  *n_fall = nl;
}

// The arguments of ww_ctc_score_trigger_bank_step (include/wwhip.h): 0, or -1 with nothing touched
static inline int sc_check_score_trigger(int64_t S, int64_t K, const void *is_speech, const void *is_active, const void *scores, const int32_t *n_post,
                                         const void *thresholds, const void *was_speech, const void *fired_ids, const void *fired_slot,
                                         const void *n_fired, const void *fall_ids, const void *n_fall) {
  (void)fired_slot;
  if (S < 0 || K < 1 || K > 8 || !n_fired || !n_fall || !thresholds) return -1;
  if (S > 0 && (!is_speech || !is_active || !scores || !n_post || !was_speech || !fired_ids || !fall_ids)) return -1;
  for (int64_t s = 0; s < S; ++s)
    if (n_post[s] < 0 || n_post[s] > 2) return -1;
  return 0;
}
