// ctc_occupancy.hip - ctc_occupancy_kernel: ctc_occupancy.h's forward-backward occupancy over any device posteriors [n][T][L], for K
// targets at once.
//
// ctc_score_kernel's decomposition (ctc_score.hip): a (sequence, target) pair owns a segment of P adjacent lanes, P = 2 Umax + 1
// rounded up to 4, 8, 16 or 32, pairs in sequence-major order; lane s of a segment keeps a(s) in a register, a(s - 1) and a(s - 2)
// arrive by DPP row shifts (P <= 16) or __shfl_up (P = 32), and the lane's column of y is fetched in groups ahead of the chain.
// What is new:
//   - nothing can be divided by Z before the forward pass has ended, so a lane parks its a_t in LDS: [T][256] floats of dynamic
//     LDS, a column per lane (one bank per lane of a half-wave: no conflict), 19 KB at T = 19 and the 64 KB a launch gets without
//     asking at T = 64.  Registers would need a run-time index (scratch), global memory a round trip per step.  In prefix mode the
//     lane of state 2U - 1, whose a is not live, parks the completion term e_t there instead.
//   - the backward pass walks t = T - 1 .. 0: b(s) in a register, m(s + 1) and m(s + 2) from the lanes ABOVE - row_shl DPP, or
//     __shfl_down at P = 32 - and a lane whose s + 1 or s + 2 is past state 2U selects +0, never what the shift brought it (its
//     neighbour segment's value, or its own).  The column of y is fetched again, in groups ahead of the chain, going down.
//     In prefix mode b(2U - 1) is pinned to 1 and b(2U) to 0 (ctc_occupancy.h).  g_t(s) = (a b) / Z replaces a_t in the lane's slot.
//   - behind a barrier the segment's lanes write the pair's occ [T][9] as one contiguous run from the parked g, and, only where cls
//     is asked for (a wave-uniform branch on the pointer), lane j of a segment takes classes j, j + P, ... of every step: the sum
//     over the states of that class in ascending s, every lane of the segment reading one LDS address at a time (a broadcast).
// No scratch, no atomics; every store is an ordinary vector store.  The lanes do ctc_occupancy.h's operations in that header's
// order: the kernel gives ww_ctc_occupancy_row's bits (tests/test_gpu_ctc_occupancy.py).
#include "common.h"

#include "ctc_occupancy.h"

template <int P>
__device__ __forceinline__ float co_shr1(float v) {
  if constexpr (P <= 16) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));  // row_shr:1
  else return __shfl_up(v, 1, 64);
}
template <int P>
__device__ __forceinline__ float co_shr2(float v) {
  if constexpr (P <= 16) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, true));  // row_shr:2
  else return __shfl_up(v, 2, 64);
}
// lane l <- lane l + 1 / l + 2.  What the top lanes of a segment receive is not used: the caller selects.
template <int P>
__device__ __forceinline__ float co_shl1(float v) {
  if constexpr (P <= 16) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x101, 0xf, 0xf, true));  // row_shl:1
  else return __shfl_down(v, 1, 64);
}
template <int P>
__device__ __forceinline__ float co_shl2(float v) {
  if constexpr (P <= 16) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x102, 0xf, 0xf, true));  // row_shl:2
  else return __shfl_down(v, 2, 64);
}

// For sequence i < n and target k < tg.K, at o = k * stride_k + i * stride_i: value[o], occ[o][T][9] and, where cls is not nullptr,
// cls[o][T][L] ([K][n] planes with strides (n, 1)).  Dynamic LDS: T * 256 floats.
template <int P>
__global__ __launch_bounds__(256) void ctc_occupancy_kernel(const float *__restrict__ steps, long long n, int T, int L, ww_ctc_score_targets tg,
                                                            float *__restrict__ value, float *__restrict__ occ, float *__restrict__ cls_out,
                                                            long long stride_k, long long stride_i) {
  extern __shared__ float park[];  // [T][256]: a_t, then g_t, a column per lane
  constexpr int PER = 256 / P;     // pairs per workgroup
  constexpr int NU = WW_CTC_SCORE_MAX_TARGET;
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
  bool skip = false, skip_up = false;  // skip(s), skip(s + 2)
  if (on && (s & 1)) {
    const int u = (s - 1) >> 1;
    cls = tg.c[k][u];
    skip = u >= 1 && tg.c[k][u] != tg.c[k][u - 1];
    skip_up = u + 1 < U && tg.c[k][u + 1] != tg.c[k][u];
  }
  const bool up1 = s + 1 < S;  // state s + 1 exists
  const bool prefix = tg.mode == WW_CTC_SCORE_PREFIX;
  const bool e_lane = prefix && s == S - 2;
  const float *col = steps + (size_t)i * T * L + cls;
  float *mine = park + tid;
  float y = col[0];
  float a = (on && s <= 1) ? y : 0.0f;
  float pre = (U == 1 && s == 1) ? y : 0.0f;  // P_t, on the lane of state 2U - 1
  mine[0] = e_lane ? pre : a;
  // (the prefetch is ctc_score_kernel's: the column a group ahead of the chain, a step past T - 1 reads row T - 1 and is dropped)
  constexpr int CO_AHEAD = 8;
  float nxt[CO_AHEAD], cur[CO_AHEAD];
#pragma unroll
  for (int j = 0; j < CO_AHEAD; ++j) nxt[j] = col[(size_t)(1 + j < T ? 1 + j : T - 1) * L];
  for (int t0 = 1; t0 < T; t0 += CO_AHEAD) {
#pragma unroll
    for (int j = 0; j < CO_AHEAD; ++j) cur[j] = nxt[j];
    if (t0 + CO_AHEAD < T) {
#pragma unroll
      for (int j = 0; j < CO_AHEAD; ++j) nxt[j] = col[(size_t)(t0 + CO_AHEAD + j < T ? t0 + CO_AHEAD + j : T - 1) * L];
    }
#pragma unroll
    for (int j = 0; j < CO_AHEAD; ++j) {
      if (t0 + j < T) {
        y = cur[j];
        float a1 = co_shr1<P>(a), a2 = co_shr2<P>(a);
        a1 = s >= 1 ? a1 : 0.0f;
        a2 = skip ? a2 : 0.0f;
        const float e = ww_cs_mul(ww_cs_add(a1, a2), y);  // on the lane of state 2U - 1: the completion term e_t
        if (prefix) pre = ww_cs_add(pre, e);
        const float nw = ww_cs_mul(ww_cs_add(ww_cs_add(a, a1), a2), y);
        a = on ? nw : 0.0f;
        mine[(t0 + j) * 256] = e_lane ? e : a;
      }
    }
  }
  const float exact = ww_cs_add(a, co_shr1<P>(a));  // on the lane of state 2U: a(2U) + a(2U - 1)
  const float Z = __shfl(prefix ? pre : exact, prefix ? S - 2 : S - 1, P);
  const bool none = Z == 0.0f;

  // the backward pass: b_{T-1}, then for t = T - 1 .. 1 m_t = b_t * y_t and b_{t-1}; g_t takes a_t's place as it goes
  float b = (on && (s == S - 2 || (s == S - 1 && !prefix))) ? 1.0f : 0.0f;
  {
    const float g = ww_cs_div(ww_cs_mul(mine[(T - 1) * 256], b), Z);
    mine[(T - 1) * 256] = none ? 0.0f : g;
  }
#pragma unroll
  for (int j = 0; j < CO_AHEAD; ++j) nxt[j] = col[(size_t)(T - 1 - j >= 0 ? T - 1 - j : 0) * L];
  for (int t0 = T - 1; t0 >= 1; t0 -= CO_AHEAD) {
#pragma unroll
    for (int j = 0; j < CO_AHEAD; ++j) cur[j] = nxt[j];
    if (t0 - CO_AHEAD >= 1) {
#pragma unroll
      for (int j = 0; j < CO_AHEAD; ++j) nxt[j] = col[(size_t)(t0 - CO_AHEAD - j >= 0 ? t0 - CO_AHEAD - j : 0) * L];
    }
#pragma unroll
    for (int j = 0; j < CO_AHEAD; ++j) {
      const int t = t0 - j;  // b is b_t; this step makes b_{t-1} and g_{t-1}
      if (t >= 1) {
        const float m = ww_cs_mul(b, cur[j]);
        float m1 = co_shl1<P>(m), m2 = co_shl2<P>(m);
        m1 = up1 ? m1 : 0.0f;
        m2 = skip_up ? m2 : 0.0f;
        const float nb = ww_cs_add(ww_cs_add(m, m1), m2);
        b = on ? nb : 0.0f;
        if (prefix) b = s == S - 2 ? 1.0f : s == S - 1 ? 0.0f : b;
        const float g = ww_cs_div(ww_cs_mul(mine[(t - 1) * 256], b), Z);
        mine[(t - 1) * 256] = none ? 0.0f : g;
      }
    }
  }
  __syncthreads();  // the lanes below read their segment's columns

  const long long o = (long long)k * stride_k + i * stride_i;
  const float *seg = park + (tid - s);
  if (live) {
    if (s == 0) value[o] = Z;
    float *po = occ + (size_t)o * T * NU;
    for (int idx = s; idx < T * NU; idx += P) {
      const int t = idx / NU, u = idx - t * NU;
      po[idx] = u < U ? seg[t * 256 + 2 * u + 1] : 0.0f;
    }
  }
  if (cls_out) {
    constexpr int SMAX = P - 1 < 2 * NU + 1 ? P - 1 : 2 * NU + 1;  // the states a segment of P lanes can hold
    int cS[SMAX];
#pragma unroll
    for (int q = 0; q < SMAX; ++q) cS[q] = __shfl(on ? cls : -1, q, P);
    float *pc = cls_out + (size_t)o * T * L;
    for (int t = 0; t < T; ++t) {
      for (int c = s; c < L; c += P) {
        float acc = 0.0f;
        bool have = false;
#pragma unroll
        for (int q = 0; q < SMAX; ++q) {
          const float g = seg[t * 256 + q];
          if (cS[q] == c) acc = have ? ww_cs_add(acc, g) : g, have = true;
        }
        if (live) pc[(size_t)t * L + c] = acc;
      }
    }
  }
}

int ww_k_ctc_occupancy(ww_ctx *ctx, const float *d_steps, int64_t n, int T, int L, const ww_ctc_score_targets &tg, float *d_value, float *d_occ,
                       float *d_cls, int64_t stride_k, int64_t stride_i) {
  if (n <= 0) return WW_OK;
  int umax = 1;
  for (int k = 0; k < tg.K; ++k) umax = tg.len[k] > umax ? tg.len[k] : umax;
  const int P = 2 * umax + 1 <= 4 ? 4 : 2 * umax + 1 <= 8 ? 8 : 2 * umax + 1 <= 16 ? 16 : 32;
  const int64_t blocks = (n * tg.K + 256 / P - 1) / (256 / P);
  if (blocks > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "ctc_occupancy_kernel: too many sequences in one call");
  const size_t lds = (size_t)T * 256 * sizeof(float);  // T <= 64: at most the 64 KB a launch gets without asking
  {
    ww_launch_scope scope(ctx, "ctc_occupancy_kernel");
#define CO_LAUNCH(P_) \
  hipLaunchKernelGGL(ctc_occupancy_kernel<P_>, dim3((unsigned)blocks), dim3(256), lds, ctx->stream, d_steps, (long long)n, T, L, tg, d_value, d_occ, \
                     d_cls, (long long)stride_k, (long long)stride_i)
    if (P == 4) CO_LAUNCH(4);
    else if (P == 8) CO_LAUNCH(8);
    else if (P == 16) CO_LAUNCH(16);
    else CO_LAUNCH(32);
#undef CO_LAUNCH
  }
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}
