// ctc_align.hip - ctc_align_kernel: ctc_align.h's Viterbi alignment over any device posteriors [n][T][L], for K targets at once.
//
// ctc_score_kernel's decomposition (ctc_score.hip): a (sequence, target) pair owns a segment of P adjacent lanes, P = 2 Umax + 1
// rounded up to 4, 8, 16 or 32, pairs in sequence-major order; lane s of a segment keeps v(s) in a register, v(s - 1) and v(s - 2)
// arrive by DPP row shifts (P <= 16) or __shfl_up (P = 32), and the lane's column of y is fetched in groups ahead of the chain.
// What is new:
//   - a lane keeps its own back-pointers in registers, 2 bits a step: step t sits in bits 2 ((t - 1) & 15) of word (t - 1) >> 4,
//     four words for T <= 64.  The forward loop gathers a group's 8 shifts with constant bit positions and ORs them into the word
//     that a wave-uniform index selects; the back-trace walks the four words in an unrolled loop.  No register is indexed at run time.
//   - the lane of state 2U - 1 tracks q, t* and its shift in prefix mode.
//   - the back-trace is T - 1 wave-uniform steps: the segment's current state is held by all of its lanes, the owning lane's
//     back-pointer comes by a segment-relative shuffle, and an odd lane notes the step when the path sits on it.  A segment whose
//     trace starts below T - 1 (prefix mode) is predicated off until its step comes.
// No LDS, no scratch, no atomics; every store is an ordinary vector store.  The lanes do ctc_align.h's comparisons and its one
// multiplication per step in that header's order: the kernel gives ww_ctc_align_row's bits (tests/test_gpu_ctc_align.py).
#include "common.h"

#include "ctc_align.h"

template <int P>
__device__ __forceinline__ float ca_shr1(float v) {
  if constexpr (P <= 16) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));  // row_shr:1
  else return __shfl_up(v, 1, 64);
}
template <int P>
__device__ __forceinline__ float ca_shr2(float v) {
  if constexpr (P <= 16) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, true));  // row_shr:2
  else return __shfl_up(v, 2, 64);
}

// For sequence i < n and target k < tg.K, at o = k * stride_k + i * stride_i: value[o] and the 18 bytes span[18 o ..]
// ([K][n] planes with strides (n, 1), a bank's [windows][K] with (1, K)).
template <int P>
__global__ __launch_bounds__(256) void ctc_align_kernel(const float *__restrict__ steps, long long n, int T, int L, ww_ctc_score_targets tg,
                                                        float *__restrict__ value, int8_t *__restrict__ span, long long stride_k,
                                                        long long stride_i) {
  constexpr int PER = 256 / P;  // pairs per workgroup
  const int tid = threadIdx.x, s = tid & (P - 1);
  const long long total = n * tg.K;
  long long pair = (long long)blockIdx.x * PER + tid / P;
  const bool live = pair < total;
  if (!live) pair = total - 1;  // (a segment past the end repeats the last pair's work and stores nothing)
  const long long i = pair / tg.K;
  const int k = (int)(pair - i * tg.K);
  const int U = tg.len[k], S = 2 * U + 1;
  const bool on = s < S;  // the segment's lanes past state 2U hold 0 throughout
  int cls = L - 1;
  bool skip = false;
  if (on && (s & 1)) {
    const int u = (s - 1) >> 1;
    cls = tg.c[k][u];
    skip = u >= 1 && tg.c[k][u] != tg.c[k][u - 1];
  }
  const bool prefix = tg.mode == WW_CTC_SCORE_PREFIX;
  const float *col = steps + (size_t)i * T * L + cls;
  float y = col[0];
  float v = (on && s <= 1) ? y : 0.0f;
  float Q = (U == 1 && s == 1) ? y : 0.0f;  // on the lane of state 2U - 1: the largest q_t, its step and its shift
  int t_star = 0, q_shift = 0;
  unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;  // the lane's back-pointers
  // (the prefetch is ctc_score_kernel's: the column a group ahead of the chain, a step past T - 1 reads row T - 1 and is dropped)
  constexpr int CA_AHEAD = 8;
  float nxt[CA_AHEAD], cur[CA_AHEAD];
#pragma unroll
  for (int j = 0; j < CA_AHEAD; ++j) nxt[j] = col[(size_t)(1 + j < T ? 1 + j : T - 1) * L];
  for (int t0 = 1; t0 < T; t0 += CA_AHEAD) {
#pragma unroll
    for (int j = 0; j < CA_AHEAD; ++j) cur[j] = nxt[j];
    if (t0 + CA_AHEAD < T) {
#pragma unroll
      for (int j = 0; j < CA_AHEAD; ++j) nxt[j] = col[(size_t)(t0 + CA_AHEAD + j < T ? t0 + CA_AHEAD + j : T - 1) * L];
    }
    unsigned g = 0;  // the group's shifts, step t0 + j in bits 2 j
#pragma unroll
    for (int j = 0; j < CA_AHEAD; ++j) {
      if (t0 + j < T) {
        y = cur[j];
        const float a1 = ca_shr1<P>(v), a2 = ca_shr2<P>(v);
        if (prefix) {  // (of use on the lane of state 2U - 1, where a1 = v(2U - 2), a2 = v(2U - 3) and y = y_t[c_{U-1}])
          float m = a1;
          int sh = 1;
          if (skip && a2 > m) m = a2, sh = 2;
          const float q = ww_cs_mul(m, y);
          if (q > Q) Q = q, t_star = t0 + j, q_shift = sh;
        }
        float best = v;
        unsigned sh = 0;
        if (s >= 1 && a1 > best) best = a1, sh = 1;
        if (skip && a2 > best) best = a2, sh = 2;
        g |= sh << (2 * j);
        const float nw = ww_cs_mul(best, y);
        v = on ? nw : 0.0f;
      }
    }
    // t0 - 1 is a multiple of 8: the group is the low or the high half of word (t0 - 1) >> 4 (wave-uniform)
    g <<= ((t0 - 1) & 8) * 2;
    const int wi = (t0 - 1) >> 4;
    w0 |= wi == 0 ? g : 0u;
    w1 |= wi == 1 ? g : 0u;
    w2 |= wi == 2 ? g : 0u;
    w3 |= wi == 3 ? g : 0u;
  }
  // where the trace starts: state st at step t_from, the value of the path
  int st, t_from, first = -1, last = -1;
  float val;
  if (prefix) {
    val = __shfl(Q, S - 2, P);
    const int ts = __shfl(t_star, S - 2, P);
    st = S - 2 - __shfl(q_shift, S - 2, P);
    t_from = ts - 1;
    if (s == S - 2) first = last = ts;
  } else {
    const int up = v > ca_shr1<P>(v) ? 1 : 0;  // on the lane of state 2U: v(2U) > v(2U - 1)
    st = S - 2 + __shfl(up, S - 1, P);
    val = __shfl(v, st, P);
    t_from = T - 1;
  }
  const unsigned w[4] = {w0, w1, w2, w3};
#pragma unroll
  for (int wi = 3; wi >= 0; --wi) {
    if (wi * 16 + 1 < T) {
      for (int j = 15; j >= 0; --j) {
        const int t = wi * 16 + 1 + j;
        if (t < T) {
          const int mine = (int)((w[wi] >> (2 * j)) & 3u);
          const int sh = __shfl(mine, st, P);
          if (t <= t_from) {
            if (s == st) {
              last = last < 0 ? t : last;
              first = t;
            }
            st -= sh;
          }
        }
      }
    }
  }
  if (t_from >= 0 && s == st) {
    last = last < 0 ? 0 : last;
    first = 0;
  }
  if (!live) return;
  const long long o = (long long)k * stride_k + i * stride_i;
  int8_t *sp = span + o * (2 * WW_CTC_SCORE_MAX_TARGET);
  if (on && (s & 1)) {
    const bool none = val == 0.0f;
    sp[s - 1] = (int8_t)(none ? -1 : first);
    sp[s] = (int8_t)(none ? -1 : last);
  }
  for (int u = U + s; u < WW_CTC_SCORE_MAX_TARGET; u += P) sp[2 * u] = sp[2 * u + 1] = -1;
  if (s == S - 2) value[o] = val;
}

int ww_k_ctc_align(ww_ctx *ctx, const float *d_steps, int64_t n, int T, int L, const ww_ctc_score_targets &tg, float *d_value, int8_t *d_span,
                   int64_t stride_k, int64_t stride_i) {
  if (n <= 0) return WW_OK;
  int umax = 1;
  for (int k = 0; k < tg.K; ++k) umax = tg.len[k] > umax ? tg.len[k] : umax;
  const int P = 2 * umax + 1 <= 4 ? 4 : 2 * umax + 1 <= 8 ? 8 : 2 * umax + 1 <= 16 ? 16 : 32;
  const int64_t blocks = (n * tg.K + 256 / P - 1) / (256 / P);
  if (blocks > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "ctc_align_kernel: too many sequences in one call");
  {
    ww_launch_scope scope(ctx, "ctc_align_kernel");
#define CA_LAUNCH(P_) \
  hipLaunchKernelGGL(ctc_align_kernel<P_>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_steps, (long long)n, T, L, tg, d_value, d_span, \
                     (long long)stride_k, (long long)stride_i)
    if (P == 4) CA_LAUNCH(4);
    else if (P == 8) CA_LAUNCH(8);
    else if (P == 16) CA_LAUNCH(16);
    else CA_LAUNCH(32);
#undef CA_LAUNCH
  }
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}
