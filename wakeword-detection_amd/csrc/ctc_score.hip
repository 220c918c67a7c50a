// ctc_score.hip - ctc_score_kernel: ctc_score.h's forward algorithm over any device posteriors [n][T][L], for K targets at once.
//
// The work is state-parallel.  A (sequence, target) pair owns a segment of P adjacent lanes, P = 2 Umax + 1 rounded up to 4, 8, 16 or
// 32 (Umax: the longest target of the call), 64 / P pairs per wave, pairs in sequence-major order (the K segments of a sequence sit
// side by side and read the same rows).  Lane s of a segment keeps a(s) in a register; a(s - 1) and a(s - 2) arrive from the two
// lanes below it - DPP row shifts where a segment lies inside a row of 16 lanes, ds_bpermute (__shfl_up) for P = 32 - and the lane
// reads its own class of the step's row, so a row is fetched once per segment.  That is a chain of T steps, not T (2U + 1); no LDS,
// no scratch.  Every lane does ctc_score.h's operations (ww_cs_add / ww_cs_mul) in that header's order: the kernel gives the bits of
// ww_ctc_score_row, which is the contract (tests/test_gpu_ctc_score.py compares them).
//
// The targets travel in the kernel's arguments (ww_ctc_score_targets, 88 bytes): nothing to upload, nothing on the stream to order
// the launch against, and the same launch serves a stream bank's tick.
#include "common.h"

#include "ctc_score.h"

// lane l <- lane l - 1 / l - 2.  What a segment's lane 0 (and lane 1) receive is not used: the caller selects.
template <int P>
__device__ __forceinline__ float cs_shr1(float v) {
  if constexpr (P <= 16) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));  // row_shr:1
  else return __shfl_up(v, 1, 64);
}
template <int P>
__device__ __forceinline__ float cs_shr2(float v) {
  if constexpr (P <= 16) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, true));  // row_shr:2
  else return __shfl_up(v, 2, 64);
}

// score[k * stride_k + i * stride_i] for sequence i < n and target k < tg.K: [K][n] planes with (n, 1), a bank's [windows][K] with (1, K)
template <int P>
__global__ __launch_bounds__(256) void ctc_score_kernel(const float *__restrict__ steps, long long n, int T, int L, ww_ctc_score_targets tg,
                                                        float *__restrict__ score, long long stride_k, long long stride_i) {
  constexpr int PER = 256 / P;  // pairs per workgroup
  const int tid = threadIdx.x, s = tid & (P - 1);
  const long long total = n * tg.K;
  long long pair = (long long)blockIdx.x * PER + tid / P;
  const bool live = pair < total;
  if (!live) pair = total - 1;  // (a segment past the end repeats the last pair's reads and stores nothing)
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
  const float *col = steps + (size_t)i * T * L + cls;
  float y = col[0];
  float a = (on && s <= 1) ? y : 0.0f;
  float pre = (U == 1 && s == 1) ? y : 0.0f;  // P_t, on the lane of state 2U - 1
  const bool prefix = tg.mode == WW_CTC_SCORE_PREFIX;
  // The lane's column of y does not depend on the recurrence: it is fetched CS_AHEAD steps at a time, a group ahead of the group
  // the chain is working through, so the chain waits for memory once and not T times (a step index past T - 1 reads row T - 1
  // again and its value is dropped: T is wave-uniform, the branches below are scalar).
  constexpr int CS_AHEAD = 8;
  float nxt[CS_AHEAD], cur[CS_AHEAD];
#pragma unroll
  for (int j = 0; j < CS_AHEAD; ++j) nxt[j] = col[(size_t)(1 + j < T ? 1 + j : T - 1) * L];
  for (int t0 = 1; t0 < T; t0 += CS_AHEAD) {
#pragma unroll
    for (int j = 0; j < CS_AHEAD; ++j) cur[j] = nxt[j];
    if (t0 + CS_AHEAD < T) {
#pragma unroll
      for (int j = 0; j < CS_AHEAD; ++j) nxt[j] = col[(size_t)(t0 + CS_AHEAD + j < T ? t0 + CS_AHEAD + j : T - 1) * L];
    }
#pragma unroll
    for (int j = 0; j < CS_AHEAD; ++j) {
      if (t0 + j < T) {
        y = cur[j];
        float a1 = cs_shr1<P>(a), a2 = cs_shr2<P>(a);
        a1 = s >= 1 ? a1 : 0.0f;
        a2 = skip ? a2 : 0.0f;
        if (prefix) pre = ww_cs_add(pre, ww_cs_mul(ww_cs_add(a1, a2), y));
        const float nw = ww_cs_mul(ww_cs_add(ww_cs_add(a, a1), a2), y);
        a = on ? nw : 0.0f;
      }
    }
  }
  const float exact = ww_cs_add(a, cs_shr1<P>(a));  // on the lane of state 2U: a(2U) + a(2U - 1)
  if (live && s == (prefix ? S - 2 : S - 1)) score[(long long)k * stride_k + i * stride_i] = prefix ? pre : exact;
}

int ww_k_ctc_score(ww_ctx *ctx, const float *d_steps, int64_t n, int T, int L, const ww_ctc_score_targets &tg, float *d_score, int64_t stride_k,
                   int64_t stride_i) {
  if (n <= 0) return WW_OK;
  int umax = 1;
  for (int k = 0; k < tg.K; ++k) umax = tg.len[k] > umax ? tg.len[k] : umax;
  const int P = 2 * umax + 1 <= 4 ? 4 : 2 * umax + 1 <= 8 ? 8 : 2 * umax + 1 <= 16 ? 16 : 32;
  const int64_t blocks = (n * tg.K + 256 / P - 1) / (256 / P);
  if (blocks > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "ctc_score_kernel: too many sequences in one call");
  {
    ww_launch_scope scope(ctx, "ctc_score_kernel");
#define CS_LAUNCH(P_) \
  hipLaunchKernelGGL(ctc_score_kernel<P_>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_steps, (long long)n, T, L, tg, d_score, \
                     (long long)stride_k, (long long)stride_i)
    if (P == 4) CS_LAUNCH(4);
    else if (P == 8) CS_LAUNCH(8);
    else if (P == 16) CS_LAUNCH(16);
    else CS_LAUNCH(32);
#undef CS_LAUNCH
  }
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}
