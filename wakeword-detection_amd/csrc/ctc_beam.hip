// ctc_beam.hip - ctc_beam_kernel: ctc_beam.h's prefix beam search over any device posteriors [n][T][L].
//
// One wave per sequence, four sequences per workgroup; lane j is beam slot j (W <= 64), and the beam lives in the lanes' registers in
// the statement's order (slot 0 the most probable).  The sequence's T L <= 152 posteriors are fetched into LDS up front.  A step:
//   1. every lane publishes (key, pb, tot) and clears its row of the claim table;
//   2. a lane whose prefix is not empty looks for its parent's key among the nb keys (LDS broadcast reads), adds that parent's
//      extension to its own stay term - the statement's ONE addition - and marks claim[parent][its last label]: B has one parent and
//      keys are distinct, so every claim byte has one writer;
//   3. every lane produces its stay candidate and its L - 1 extensions, the claimed ones and the slots past nb or past L - 1 as
//      (-Inf, WW_CB_NO_KEY), which nothing real comes after - at most 8 x 64 candidates (rank, key) in LDS, the values in registers;
//   4. selection is rank by counting: a lane counts, for each of its candidates, the candidates that come before it in the
//      statement's total order (ww_cb_before; the others arrive as broadcast reads), and that count IS the candidate's slot in the
//      next beam - a candidate whose count is under min(W, candidates) stores itself there, and every lane reads its new slot.
// LDS is ordered wave-synchronously (the LDS instructions of one wave execute in issue order; cb_sync only stops the compiler): no
// workgroup barrier, no atomics, no scratch.  Every arithmetic operation and every comparison is one of ctc_beam.h's functions, so
// the kernel gives ww_ctc_beam_row's bits (tests/test_gpu_ctc_beam.py compares them).  A wave past n repeats the last sequence's
// reads and stores nothing.
#include "common.h"

#include "ctc_beam.h"

#define CB_WAVES 4  // sequences per workgroup
#define CB_Q WW_CTC_BEAM_MAX_L  // candidates per lane: the stay and up to 7 extensions

struct cb_wave {
  uint64_t key[64];
  uint64_t claim[64];  // byte c of word p: label c of slot p's extensions is taken by a beam entry
  uint64_t ckey[CB_Q][64];
  float crank[CB_Q][64];
  float pb[64], pnb[64], tot[64];
  float y[WW_CTC_BEAM_MAX_T * WW_CTC_BEAM_MAX_L];
};

__device__ __forceinline__ void cb_sync() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Q: the candidates a lane can hold, L rounded up to 2, 4 or 8 - the loops over a lane's candidates are unrolled to it
template <int Q>
__global__ __launch_bounds__(64 * CB_WAVES) void ctc_beam_kernel(const float *__restrict__ steps, long long n, int T, int L, int W, int P, int max_labels,
                                                                 int32_t *__restrict__ labels, int32_t *__restrict__ lengths, float *__restrict__ prob) {
  __shared__ cb_wave sm[CB_WAVES];
  const int lane = threadIdx.x & 63;
  cb_wave &s = sm[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
  long long seq = (long long)blockIdx.x * CB_WAVES + (threadIdx.x >> 6);
  const bool live = seq < n;
  if (!live) seq = n - 1;
  const float *y = steps + (size_t)seq * T * L;
  for (int i = lane; i < T * L; i += 64) s.y[i] = y[i];
  const int blank = L - 1;
  uint64_t key = lane == 0 ? 0 : WW_CB_NO_KEY;
  float pb = lane == 0 ? 1.0f : 0.0f, pnb = 0.0f;
  int nb = 1;
  cb_sync();
  for (int t = 0; t < T; ++t) {
    const float *row = s.y + t * L;
    const bool on = lane < nb;
    const int last = on ? ww_cb_last(key) : -1;
    const float tot = ww_cb_tot(pb, pnb);
    const float st_pb = ww_cb_stay_pb(tot, row[blank]);
    float st_pnb = ww_cb_stay_pnb(pnb, last, row[last < 0 ? 0 : last]);
    s.key[lane] = key;
    s.pb[lane] = pb;
    s.tot[lane] = tot;
    s.claim[lane] = 0;
    cb_sync();
    // 2. the parent, if the beam holds it
    const uint64_t pk = last >= 0 ? ww_cb_parent(key) : WW_CB_NO_KEY;
    int par = -1;
    for (int i = 0; i < nb; ++i) par = s.key[i] == pk ? i : par;
    if (par >= 0) {
      st_pnb = ww_cb_merge(st_pnb, ww_cb_ext(s.pb[par], s.tot[par], ww_cb_last(pk), last, row[last]));
      ((uint8_t *)s.claim)[par * 8 + last] = 1;
    }
    cb_sync();
    const uint64_t claimed = s.claim[lane];
    // 3. the lane's candidates: [0] the stay, [1 + c] the extension by label c
    float r[Q], cpnb[Q];
    uint64_t k[Q];
    r[0] = on ? ww_cb_rank(ww_cb_tot(st_pb, st_pnb)) : -__builtin_inff();
    k[0] = on ? key : WW_CB_NO_KEY;
    cpnb[0] = st_pnb;
    int ncand = __popcll(__ballot(on));
#pragma unroll
    for (int c = 0; c < Q - 1; ++c) {
      const bool valid = on && c < blank && !((claimed >> (8 * c)) & 0xff);
      const float e = ww_cb_ext(pb, tot, last, c, row[c < blank ? c : 0]);
      cpnb[1 + c] = e;
      r[1 + c] = valid ? ww_cb_rank(ww_cb_tot(0.0f, e)) : -__builtin_inff();
      k[1 + c] = valid ? ww_cb_append(on ? key : 0, c) : WW_CB_NO_KEY;
      ncand += __popcll(__ballot(valid));
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (q < L) {
        s.crank[q][lane] = r[q];
        s.ckey[q][lane] = k[q];
      }
    cb_sync();
    // 4. rank by counting
    int cnt[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) cnt[q] = 0;
    for (int q2 = 0; q2 < L; ++q2)
      for (int i = 0; i < nb; ++i) {
        const float orank = s.crank[q2][i];
        const uint64_t okey = s.ckey[q2][i];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          cnt[q] += ww_cb_before(orank, okey, r[q], k[q]) ? 1 : 0;
          __builtin_amdgcn_sched_barrier(0);  // one candidate's compare masks at a time: eight at once spill scalar registers
        }
      }
    const int nb_new = ncand < W ? ncand : W;
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (k[q] != WW_CB_NO_KEY && cnt[q] < nb_new) {
        s.key[cnt[q]] = k[q];
        s.pb[cnt[q]] = q == 0 ? st_pb : 0.0f;
        s.pnb[cnt[q]] = cpnb[q];
      }
    cb_sync();
    nb = __builtin_amdgcn_readfirstlane(nb_new);
    const bool on2 = lane < nb;
    key = on2 ? s.key[lane] : WW_CB_NO_KEY;
    pb = on2 ? s.pb[lane] : 0.0f;
    pnb = on2 ? s.pnb[lane] : 0.0f;
    cb_sync();
  }
  if (live && lane < P) {
    const bool have = lane < nb;
    ww_cb_report(have, have ? key : 0, pb, pnb, max_labels, labels + ((size_t)seq * P + lane) * max_labels, lengths + (size_t)seq * P + lane,
                 prob + (size_t)seq * P + lane);
  }
}

int ww_k_ctc_beam(ww_ctx *ctx, const float *d_steps, int64_t n, int T, int L, int W, int P, int max_labels, int32_t *d_labels, int32_t *d_lengths,
                  float *d_prob) {
  if (n <= 0) return WW_OK;
  const int64_t blocks = (n + CB_WAVES - 1) / CB_WAVES;
  if (blocks > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "ctc_beam_kernel: too many sequences in one call");
  {
    ww_launch_scope scope(ctx, "ctc_beam_kernel");
#define CB_LAUNCH(Q_) \
  hipLaunchKernelGGL(ctc_beam_kernel<Q_>, dim3((unsigned)blocks), dim3(64 * CB_WAVES), 0, ctx->stream, d_steps, (long long)n, T, L, W, P, max_labels, \
                     d_labels, d_lengths, d_prob)
    if (L <= 2) CB_LAUNCH(2);
    else if (L <= 4) CB_LAUNCH(4);
    else CB_LAUNCH(8);
#undef CB_LAUNCH
  }
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}
