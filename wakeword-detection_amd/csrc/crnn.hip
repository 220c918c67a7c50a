// CRNN encode + detect for gfx950 (fp32, MFMA for the dense contractions).
//
// Replaces encode.tflite + detect.tflite of the reference CRNN
// (tf_lite_models/CRNN; architecture wwdetect/CRNN/model.py:21-56; call sites
// spokestack/wakeword/tflite.py:193-231, utils/evaluate_models.py:76-80).
//
//   crnn_fused_kernel  the whole model for one window in one 4-wave workgroup: Conv2D(1->32, 5x20, stride 2x8, SAME,
//                      ReLU) as an implicit GEMM, the layer-1 input projections of both GRU directions (K = 640,
//                      N = 192), both bidirectional GRU layers and the detect head - nothing between the mel window
//                      and the posterior leaves the CU (header of the kernel below).
//   generic path       any other conv geometry (utils/CRNN_files/*_old.tflite): conv_generic_kernel, gemm_nt_kernel
//                      (C = A W^T + b, 64x64x64 tiles, fp32 MFMA, XCD-aware tile order), gru_generic_kernel,
//                      crnn_detect_kernel.
//   other cells        an LSTM, a GRU of 16, 48 or 64 units, a head of another width than 64 (what the trainer's tuner can pick):
//                      the generic path with rnn_layer_kernel<CELL, H> for the recurrences and crnn_head_kernel for the head,
//                      whatever the conv geometry.
// Round 1's three-kernel chain (conv5x20_kernel -> gemm_nt_kernel -> gru_head_kernel, 52 us per 256 windows against
// 34 us fused) and its bf16x6 projection GEMM are gone; their measurements are in DESIGN.md 7.1.
#include "stream_fe.h"
#include "ctc_decode.h"
#include "stream_ctc.h"
#include <algorithm>
#include <type_traits>

#include <cstdlib>

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct win_addr {
  const int64_t *row;    // explicit first mel row per window, or nullptr
  const int32_t *valid;  // explicit valid rows per window, or nullptr
  int64_t row0;
  int hop;
  int valid_const;
  int64_t mel_rows;
};

__device__ __forceinline__ void window_span(const win_addr &wa, int w, int T, int64_t &row, int &valid) {
  if (wa.row && wa.valid) {  // (both tables: the two loads go out together, one round trip at the head of the kernel)
    const int64_t r = wa.row[w];
    const int v = wa.valid[w];
    row = r;
    valid = v;
  } else {
    row = wa.row ? wa.row[w] : wa.row0 + (int64_t)w * wa.hop;
    valid = wa.valid ? wa.valid[w] : wa.valid_const;
  }
  if (valid > T) valid = T;
  if (row + valid > wa.mel_rows) valid = (int)(wa.mel_rows - row);
  if (valid < 0) valid = 0;
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// The detect head's activation for output o of a window: sigmoid (HEAD == 0), or softmax over the NOUT <= 8 outputs, which sit in
// eight adjacent lanes (o = lane % 8; lanes with o >= NOUT take part in the exchanges and return nothing of use).  Every lane of
// the wave calls it.
__device__ __forceinline__ float head_activation(float y, int o, int NOUT, int HEAD) {
  if (HEAD == 0) return sigmoid_f(y);
  float mx = (o < NOUT) ? y : -INFINITY;
  for (int d = 1; d < 8; d <<= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  const float e = (o < NOUT) ? expf(y - mx) : 0.f;
  float sum = e;
  for (int d = 1; d < 8; d <<= 1) sum += __shfl_xor(sum, d);
  return e / sum;
}

// LDS clear by a workgroup of threads_ (thread tid): n4_ x 16 bytes from p_ (the window image).  This and CLEAR_SEQ_H are
// macros because as functions the unrolled loops came out with other exit branches in every kernel that uses them
// (profiles/EXPERIMENTS.md 13).
#define LDS_CLEAR16(p_, n4_, threads_) \
  for (int i = tid; i < (n4_); i += (threads_)) ((float4 *)(p_))[i] = make_float4(0.f, 0.f, 0.f, 0.f);

// Four mel features at p (zeros unless `in`).  Whether the window's first row is 16-byte aligned is uniform over a workgroup,
// so the staging loops branch on it ONCE, outside (stage_loads below): with the 16-byte and the 4 x 4-byte form behind one
// per-element condition the compiler drained the memory counter after every element's loads - six round trips to L2 in a
// row at the head of crnn_fused_kernel (6.4 k of its 72 k cycles) instead of six loads in flight.
template <bool AL16>
__device__ __forceinline__ float4 ld_mel4(const float *p, bool in) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (in) {
    if (AL16) v = *(const float4 *)p;
    else v = make_float4(p[0], p[1], p[2], p[3]);
  }
  return v;
}
// The same from an address that is readable whatever `in` says (the caller clamps it into the buffer): the load is
// unconditional - no exec masking, nothing the next load has to wait for - and `in` only selects between it and zeros.
template <bool AL16>
__device__ __forceinline__ float4 ld_mel4_sel(const float *p_safe, bool in) {
  const float4 v = ld_mel4<AL16>(p_safe, true);
  return make_float4(in ? v.x : 0.f, in ? v.y : 0.f, in ? v.z : 0.f, in ? v.w : 0.f);
}
template <typename F>
__device__ __forceinline__ void stage_loads(bool al16, F &&body) {
  if (al16) body(std::true_type{});
  else body(std::false_type{});
}

// ------------------------------------------------------------------------------------------
// conv
// ------------------------------------------------------------------------------------------
#define CV_ROWS 44   // mel index + PF, 0..43
#define CV_LDT 164   // time index + PT, 0..163 (multiple of 4; 164 % 32 == 4)
#define CV_KB 6      // K = 5*20 = 100 = 6 k-blocks of 16 and one last quad (k = 96..99): 25 MFMA k-steps, none on padding
#define CV_QL 24     // the last quad
#define CV_THREADS 512
// Geometry of every CRNN the reference ships (wwdetect/CRNN/train.py:27-49; checked against the
// blob at model load): compile-time constants turn the index divisions into shifts/multiplies.
#define CV_NMEL 40
#define CV_KF 5
#define CV_KT 20
#define CV_SF 2
#define CV_ST 8
#define CV_PF 1
#define CV_PT 6
#define CV_OF 20
#define CV_OT 19

// ------------------------------------------------------------------------------------------
// GEMM  C[M][N] = A[M][K] * W[N][K]^T + bias[N]
// ------------------------------------------------------------------------------------------
#define GB_M 64
#define GB_N 64
#ifndef GB_K
#define GB_K 64
#endif
#define GB_LD (GB_K + 8)  // 288 B rows at K = 64 (32 mod 64): the operand ds_read_b128s are bank-conflict-free (68 was 2-way conflicted)

struct gemm_args {
  const float *A;
  const float *W;
  const float *bias;
  float *C;
  int M, N, K;
  int n_tiles;  // ceil(N / 64)
};

// 512 threads = 8 waves (2 per SIMD, so one wave's LDS/MFMA latencies are covered by its partner);
// wave (wr, wc) = (wave >> 1, wave & 1) owns rows wr*16..+15, columns wc*32..+31 of the 64x64 tile.
__global__ __launch_bounds__(512) void gemm_nt_kernel(gemm_args g) {
  __shared__ __align__(16) float As[2][GB_M * GB_LD];
  __shared__ __align__(16) float Bs[2][GB_N * GB_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  // XCD-aware tile order: workgroups go round-robin to the 8 XCDs (id % 8), each with its own L2.  The n-tiles
  // of one m-tile read the same 64 rows of A, so they are given ids of equal residue: A then crosses the fabric
  // once instead of once per n-tile (FETCH_SIZE 28.9 -> see profiles/r01/pmc_traffic.json).
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int mt = (slot / g.n_tiles) * 8 + xcd, nt = slot % g.n_tiles;
  if (mt * GB_M >= g.M) return;
  const int m0 = mt * GB_M, n0 = nt * GB_N;
  constexpr int C4 = GB_K / 4, LROWS = 512 / C4, LH = GB_M / LROWS;  // loader: LH rows per thread, float4 column lc4
  const int lrow = tid / C4, lc4 = tid % C4;
  const int i16 = lane & 15, kk = lane >> 4;

  float4 pa[LH], pb[LH];
  auto gload = [&](int k0) {
#pragma unroll
    for (int h = 0; h < LH; ++h) {
      const int r = lrow + LROWS * h;
      const int gm = m0 + r;
      pa[h] = gm < g.M ? *(const float4 *)(g.A + (size_t)gm * g.K + k0 + lc4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      const int gn = n0 + r;
      pb[h] = gn < g.N ? *(const float4 *)(g.W + (size_t)gn * g.K + k0 + lc4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int h = 0; h < LH; ++h) {
      const int r = lrow + LROWS * h;
      *(float4 *)(&As[buf][r * GB_LD + lc4 * 4]) = pa[h];
      *(float4 *)(&Bs[buf][r * GB_LD + lc4 * 4]) = pb[h];
    }
  };

  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const int nk = g.K / GB_K;
  gload(0);
  sstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) gload((kt + 1) * GB_K);
#pragma unroll
    for (int kb = 0; kb < GB_K / 16; ++kb) {
      const float4 av = *(const float4 *)(&As[cur][(wr * 16 + i16) * GB_LD + kb * 16 + kk * 4]);
      const float4 b0 = *(const float4 *)(&Bs[cur][(wc * 32 + i16) * GB_LD + kb * 16 + kk * 4]);
      const float4 b1 = *(const float4 *)(&Bs[cur][(wc * 32 + 16 + i16) * GB_LD + kb * 16 + kk * 4]);
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b0.x, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b1.x, acc[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b0.y, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b1.y, acc[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, b0.z, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, b1.z, acc[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, b0.w, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, b1.w, acc[1], 0, 0, 0);
    }
    if (kt + 1 < nk) sstore(cur ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int gn = n0 + wc * 32 + ni * 16 + i16;
    const float bv = (gn < g.N) ? g.bias[gn] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gm = m0 + wr * 16 + kk * 4 + r;
      if (gm < g.M && gn < g.N) g.C[(size_t)gm * g.N + gn] = acc[ni][r] + bv;
    }
  }
}

// ------------------------------------------------------------------------------------------
// GRU building blocks (one lane pair per unit: K split over adjacent lanes, joined by one DPP swap)
// ------------------------------------------------------------------------------------------
#define GR_H 32
#define GR_SEQ_LD 68   // seq1 row: 64 values + 4 pad
#define GR_GX_LD 196   // gx2 row: 192 values + 4 pad
#define GR_W1_LD 65

// v_exp_f32 / v_rcp_f32 based gates (~1 ulp each): |error| ~ 2e-7, far inside the 1e-4 budget,
// and several times shorter than the libm expf / tanhf / IEEE-divide sequences that sit on the
// 38-step serial chain.
__device__ __forceinline__ float fast_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float fast_tanh(float x) {
  const float e = __builtin_amdgcn_exp2f(2.8853900817779268f * x);  // exp(2x): inf -> 1, 0 -> -1
  return __fmaf_rn(-2.0f, __builtin_amdgcn_rcpf(1.0f + e), 1.0f);  // spelled out: every kernel rounds it the same way
}
// The GRU cell's last two lines, spelled out (no contraction left to the compiler) so that the vector form (gru_step) and the
// matrix form (gru_tail16_kernel) round identically:  c = tanh(xc + r * hc),  h' = z h + (1 - z) c
__device__ __forceinline__ float gru_candidate(float r, float hc, float xc) { return fast_tanh(__fmaf_rn(r, hc, xc)); }
__device__ __forceinline__ float gru_blend(float z, float h, float c) { return __fmaf_rn(z, h, __fmul_rn(__fsub_rn(1.0f, z), c)); }

__device__ __forceinline__ float swap_pair(float v) {
  // value of the neighbouring lane (lane ^ 1): DPP quad_perm [1,0,3,2]
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct gru_w {
  f32x2 z[8], r[8], c[8];  // W_h rows of this lane's unit, columns [16*half, 16*half+16), as pairs
  float bz, br, bc;
};

__device__ __forceinline__ void gru_load_w(gru_w &g, const float *wh, const float *bh, int dir, int unit, int half) {
  const float *base = wh + (size_t)dir * 3 * GR_H * GR_H;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 z = *(const float4 *)(base + (size_t)(0 * GR_H + unit) * GR_H + half * 16 + q * 4);
    const float4 r = *(const float4 *)(base + (size_t)(1 * GR_H + unit) * GR_H + half * 16 + q * 4);
    const float4 c = *(const float4 *)(base + (size_t)(2 * GR_H + unit) * GR_H + half * 16 + q * 4);
    g.z[2 * q] = (f32x2){z.x, z.y}; g.z[2 * q + 1] = (f32x2){z.z, z.w};
    g.r[2 * q] = (f32x2){r.x, r.y}; g.r[2 * q + 1] = (f32x2){r.z, r.w};
    g.c[2 * q] = (f32x2){c.x, c.y}; g.c[2 * q + 1] = (f32x2){c.z, c.w};
  }
  // the recurrent biases are the initial values of half 0's odd-k chains (gru_step); half 1's chains start from zero
  g.bz = half ? 0.f : bh[dir * 3 * GR_H + unit];
  g.br = half ? 0.f : bh[dir * 3 * GR_H + GR_H + unit];
  g.bc = half ? 0.f : bh[dir * 3 * GR_H + 2 * GR_H + unit];
}

// One GRU step for lane (unit = lane >> 1, half = lane & 1).  hin: this direction's h in LDS.
// Keras GRU v2 (reset_after): z = s(xz + hz), r = s(xr + hr), c = tanh(xc + r * hc), h' = z h + (1-z) c
// ONE association for every kernel that evaluates the cell (this function: crnn_fused_kernel, gru_tail_kernel,
// crnn_stream_kernel, the generic path; gru_tail16_kernel restates it on v_mfma_f32_16x16x4_f32, whose four products are an
// fmaf chain onto the accumulator in k order - tools/mfma_order_probe.hip): a gate's pre-activation is
//     (E0 + O0) + (E1 + O1)
// with four fmaf chains over the units k of the state, eight terms each, k ascending:
//     E0: k = 0, 2, .. 14 starting from the projected input x (z, r; 0 for c)      O0: k = 1, 3, .. 15 starting from b_h
//     E1: k = 16, 18, .. 30 from 0                                                 O1: k = 17, 19, .. 31 from 0
// Here E and O are the two halves of a packed fp32 FMA (v_pk_fma_f32) and the index 0 / 1 is the lane of the pair (half);
// the halves meet through one DPP swap.  The result does not depend on which kernel a window was dispatched to.
template <bool PREFETCH>
__device__ __forceinline__ float gru_step(const gru_w &g, const float *hin, int half, float gz, float gr, float gc, float h_own,
                                          const float *gx_next, float &nz, float &nr, float &nc) {
  const float4 *hp = (const float4 *)(hin + half * 16);
  // all four reads in flight before the first product, in the order of their use (the LDS answers in issue order; left alone
  // the scheduler issues the first-needed quad last)
  float4 hv[4];
  hv[0] = hp[0];
  __builtin_amdgcn_sched_barrier(0);
  hv[1] = hp[1];
  hv[2] = hp[2];
  hv[3] = hp[3];
  __builtin_amdgcn_sched_barrier(0);
  if (PREFETCH) {  // the next step's projected inputs (LDS): behind the h reads
    nz = gx_next[0];
    nr = gx_next[GR_H];
    nc = gx_next[2 * GR_H];
  }
  f32x2 az = {half ? 0.f : gz, g.bz}, ar = {half ? 0.f : gr, g.br}, ac = {0.f, g.bc};
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x2 h0 = {hv[q].x, hv[q].y}, h1 = {hv[q].z, hv[q].w};
    // the three chains strictly round-robin (a dependent packed FMA does not issue back to back; left alone the scheduler
    // runs one chain ahead of the others: +55 cycles per step)
    az = __builtin_elementwise_fma(g.z[2 * q], h0, az); ar = __builtin_elementwise_fma(g.r[2 * q], h0, ar); ac = __builtin_elementwise_fma(g.c[2 * q], h0, ac);
    __builtin_amdgcn_sched_barrier(0);
    az = __builtin_elementwise_fma(g.z[2 * q + 1], h1, az); ar = __builtin_elementwise_fma(g.r[2 * q + 1], h1, ar); ac = __builtin_elementwise_fma(g.c[2 * q + 1], h1, ac);
    __builtin_amdgcn_sched_barrier(0);
  }
  float sz = az.x + az.y, sr = ar.x + ar.y, sc = ac.x + ac.y;
  sz += swap_pair(sz);
  sr += swap_pair(sr);
  sc += swap_pair(sc);
  const float z = fast_sigmoid(sz);
  const float r = fast_sigmoid(sr);
  return gru_blend(z, h_own, gru_candidate(r, sc, gc));
}

// The wave's number within its workgroup, in a scalar register: tid >> 6 is the same in all 64 lanes, which the compiler
// cannot know - what is derived from it (a direction, a time position, `wave < 2`) would be vector work and exec-mask forks.
__device__ __forceinline__ int wave_index(int tid) { return __builtin_amdgcn_readfirstlane(tid >> 6); }

// Between the h write of one step and the h reads of the next: LDS instructions of ONE wave are
// executed in issue order, so no s_waitcnt is needed - only the compiler must not reorder them.
__device__ __forceinline__ void wsync_h() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Workgroup barrier between LDS producers and consumers only: waits for this wave's LDS traffic, not for its outstanding
// global loads (__syncthreads() drains the memory counter too - a prefetch issued just before it is then waited for in full)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

__device__ __forceinline__ void wsync_g() {
  // LDS traffic of one wave is processed in order; wait for it only (not for outstanding
  // global loads, which an acq_rel fence would also drain) and stop compiler reordering
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// In front of the recurrences: `rows` rows of seq1 (the layer-2 projection reads zeros past row 18) and the states
// h[layer 2][dir 2][ping-pong 2][32] start from zero
#define CLEAR_SEQ_H(seq1_, rows_, hb_, threads_)                                      \
  for (int i = tid; i < (rows_) * GR_SEQ_LD; i += (threads_)) (seq1_)[i] = 0.f;       \
  for (int i = tid; i < 2 * 2 * 2 * GR_H; i += (threads_)) (hb_)[i] = 0.f;

// ------------------------------------------------------------------------------------------
// The fp32 conv as crnn_fused_kernel, crnn_stream_kernel and crnn_rows_kernel run it: an implicit GEMM on v_mfma_f32_16x16x4_f32,
// m-tiles of 16 (position, frequency) rows x 32 channels, K = 100 taps = 6 k-blocks of 16 and one quad.  One definition of each piece;
// lane (j, kk) = (lane & 15, lane >> 4) are names of the kernel.  The loads are macros, not functions: as __forceinline__
// functions that take the pointer as a parameter they lost their scalar base (global_load_dwordx4 v, v, s[2:3] became
// v_lshl_add_u64 + a load from a 64-bit vector address: profiles/EXPERIMENTS.md 13).
// ------------------------------------------------------------------------------------------
// this lane's conv weights (B operand: [CV_KPAD/4][32][4]; the last quad's k = 96 + kk is element kk of it) and the biases of its
// two channels
#define CV_LOAD_W(wreg_, wlast_, cb0_, cb1_, w4_, cbias_)                                            \
  _Pragma("unroll") for (int kb = 0; kb < CV_KB; ++kb)                                               \
    _Pragma("unroll") for (int n = 0; n < 2; ++n)                                                    \
      wreg_[kb][n] = *(const float4 *)((w4_) + ((size_t)(kb * 4 + kk) * 32 + n * 16 + j) * 4);       \
  _Pragma("unroll") for (int n = 0; n < 2; ++n)                                                      \
    wlast_[n] = (w4_)[((size_t)CV_QL * 32 + n * 16 + j) * 4 + kk];                                   \
  cb0_ = (cbias_)[j];                                                                                \
  cb1_ = (cbias_)[16 + j];
// the A operands of one m-tile: abase_ = this lane's row (position, frequency) in the transposed image.  Six k-blocks as
// 16-byte reads (lane group kk: quad 4 kb + kk) and the last quad one float per lane group
struct cv_a {
  float4 q[CV_KB];
  float last;
};
#define CV_LOAD_A(av_, abase_)                                                                       \
  _Pragma("unroll") for (int kb = 0; kb < CV_KB; ++kb) {                                             \
    const int k4 = kb * 16 + kk * 4;                                                                 \
    const int kf = k4 / CV_KT, kt = k4 - kf * CV_KT;                                                 \
    av_.q[kb] = *(const float4 *)((abase_) + kf * CV_LDT + kt);                                      \
  }                                                                                                  \
  av_.last = (abase_)[(CV_QL * 4 / CV_KT) * CV_LDT + CV_QL * 4 % CV_KT + kk];
// one k-block: 16 taps x 32 channels onto acc0 (channels 0..15) and acc1 (16..31)
#define CV_MFMA_KB(av_, kb_)                                                                         \
  acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.q[kb_].x, wreg[kb_][0].x, acc0, 0, 0, 0);           \
  acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.q[kb_].x, wreg[kb_][1].x, acc1, 0, 0, 0);           \
  acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.q[kb_].y, wreg[kb_][0].y, acc0, 0, 0, 0);           \
  acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.q[kb_].y, wreg[kb_][1].y, acc1, 0, 0, 0);           \
  acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.q[kb_].z, wreg[kb_][0].z, acc0, 0, 0, 0);           \
  acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.q[kb_].z, wreg[kb_][1].z, acc1, 0, 0, 0);           \
  acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.q[kb_].w, wreg[kb_][0].w, acc0, 0, 0, 0);           \
  acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.q[kb_].w, wreg[kb_][1].w, acc1, 0, 0, 0);
// the last quad: the k-lanes carry k = 96, 97, 98, 99.  The instruction adds its four products to the accumulator as an fmaf
// chain in k-lane order, which is the order four instructions on the elements of a 16-byte operand - one
// live k-lane each, three on the zero padding of K = 112 - added them in: the same bits for every finite input (the padding's
// zero products are gone with it: they could only turn an accumulator of -0 into +0, which needs a bias of -0, or make a NaN out
// of a non-finite mel value one row further down the image)
#define CV_MFMA_LAST(av_)                                                                            \
  acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.last, wlast[0], acc0, 0, 0, 0);                     \
  acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.last, wlast[1], acc1, 0, 0, 0);
// NT_ m-tiles per wave, software-pipelined by hand: the next tile's A operands are read while this tile's MFMAs run, and what
// the caller does with the previous tile's sums prev0 / prev1 (the statements after NT_: ReLU + store, or keep them) sits in the
// middle of them.  Vector instructions between fp32 MFMAs cost matrix time, so the loop holds none it can avoid: operand and
// store offsets are the caller's, computed during the staging, the bias is the accumulators' initial value.  The caller has
// load_a(av, i), wreg, wlast, cb0, cb1 and f32x4 prev0, prev1, which are the last tile's sums afterwards.  (As a function template
// with the middle as a callable, crnn_rows_kernel kept its instructions and crnn_fused_kernel did not: EXPERIMENTS 13.)
#define CV_TILE_LOOP(NT_, ...)                                                                       \
  {                                                                                                  \
    cv_a av[2];                                                                                      \
    load_a(av[0], 0);                                                                                \
    _Pragma("unroll") for (int i = 0; i < NT_; ++i) {                                                \
      if (i + 1 < NT_) load_a(av[(i + 1) & 1], i + 1);                                               \
      __builtin_amdgcn_sched_barrier(0);                                                             \
      f32x4 acc0 = {cb0, cb0, cb0, cb0}, acc1 = {cb1, cb1, cb1, cb1};                                \
      CV_MFMA_KB(av[i & 1], 0) CV_MFMA_KB(av[i & 1], 1) CV_MFMA_KB(av[i & 1], 2)                     \
      __builtin_amdgcn_sched_barrier(0);                                                             \
      __VA_ARGS__                                                                                    \
      __builtin_amdgcn_sched_barrier(0);                                                             \
      CV_MFMA_KB(av[i & 1], 3) CV_MFMA_KB(av[i & 1], 4) CV_MFMA_KB(av[i & 1], 5) CV_MFMA_LAST(av[i & 1]) \
      prev0 = acc0;                                                                                  \
      prev1 = acc1;                                                                                  \
    }                                                                                                \
  }

// ------------------------------------------------------------------------------------------
// The layer-1 input projection gx1 = feat x W_x1^T (K = 640 = 40 k-steps of 16, N = 192: three n-tiles of 16 columns per wave)
// as the same three kernels run it.  W_x1 streams from L2 straight into registers in B-operand order ([k/4][192][4], one
// contiguous KB per wave load) through a ring bq[DEPTH][3] that is DEPTH - 1 k-steps ahead of its use; the A operands come from
// LDS one k-step ahead (avq: the 16-row tile on v_mfma_f32_16x16x4_f32, rvq: the 3-row tile on v_mfma_f32_4x4x1_16b_f32).
// ------------------------------------------------------------------------------------------
// this lane's W_x1 operand of k-step ks, n-tile n: [ks][kk][192][4] floats, so its address is
//     (wx1s + ks * PJ_KS_BYTES)  +  (kk * 192 + wave * 48 + j) * 16  +  n * 256
//      uniform: a scalar pair,       32 bits, computed once            the load's immediate offset
// i.e. global_load_dwordx4 v, v_lane, s[base:base+1] offset:256 n, the base advanced by s_add_u32 / s_addc_u32.  Left to
// itself the compiler folds the lane part into a 64-bit vector pointer and advances THAT per k-step (the stride is past the
// immediate's range): a v_add_co_u32 / v_addc_co_u32 pair and an s_nop between the MFMAs of 36 k-steps, at matrix-time prices
// (profiles/EXPERIMENTS.md 19).  Two empty asm statements per k-step keep the parts apart - "+s" pins the base in scalar
// registers, "+v" makes the lane offset a value of the k-step's own basic block, where instruction selection can see that it
// is 32 bits wide - and the pointer says "global memory" outright, because behind the asm the compiler no longer knows where
// it came from and would fall back to flat loads.  The loads themselves stay plain C++ (the compiler counts them in vmcnt).
// (__builtin_amdgcn_raw_buffer_load_b128 would do the same with a scalar offset, but this compiler lowers it to a one-dword
//  load on gfx950: not used)
// PJ_W_LANE declares the kernel's two names (wb_0, wb_lane; kk, wave and j are the kernel's), PJ_W_KSTEP the base of one
// k-step, PJ_W_LD is the load of one n-tile from it.
#define PJ_KS_BYTES (4 * 192 * 16)
typedef const __attribute__((address_space(1))) char *pj_gptr;
typedef const __attribute__((address_space(1))) f32x4 *pj_gptr4;
__device__ __forceinline__ float4 pj_w_ld(pj_gptr4 p) {
  const f32x4 v = *p;
  return make_float4(v.x, v.y, v.z, v.w);
}
#define PJ_W_LANE(wx1s_)                                                                             \
  const pj_gptr wb_0 = (pj_gptr)(wx1s_);                                                             \
  unsigned wb_lane = (unsigned)((kk * 192 + wave * 48 + j) * 16);
#define PJ_W_KSTEP(wk_, ks_)                                                                         \
  pj_gptr wk_ = wb_0 + (size_t)(ks_) * PJ_KS_BYTES;                                                  \
  asm("" : "+s"(wk_));                                                                               \
  asm("" : "+v"(wb_lane));
#define PJ_W_LD(wk_, n_) pj_w_ld((pj_gptr4)(wk_ + wb_lane + (n_) * 256))
// the ring's first DEPTH_ - 1 k-steps: requested in front of the barrier that completes feat (it does not wait for them)
#define PJ_RING_PROLOGUE(DEPTH_)                                                                     \
  _Pragma("unroll") for (int s2 = 0; s2 < DEPTH_ - 1; ++s2) {                                        \
    PJ_W_KSTEP(wk, s2)                                                                               \
    _Pragma("unroll") for (int n = 0; n < 3; ++n) bq[s2][n] = PJ_W_LD(wk, n);                        \
  }
// the biases of this lane's three columns: requested in front of the k-loop, added when the products are complete
#define PJ_LOAD_BIAS(bv1_, bx1_)                                                                     \
  _Pragma("unroll") for (int n = 0; n < 3; ++n) bv1_[n] = (bx1_)[wave * 48 + n * 16 + j];
// one operand element e_ of a k-step on the row groups a kernel has; consecutive MFMAs go to different accumulators
// (dependent-accumulator latency 40 > issue 32).  The order of the MFMAs in a round and of the k-steps is the association of
// every sum of gx1.
#define PJ_ROWS16(e_)                                                                                \
  acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(avq[ks & 1].e_, b[0].e_, acc[0], 0, 0, 0);            \
  acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(avq[ks & 1].e_, b[1].e_, acc[1], 0, 0, 0);            \
  acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(avq[ks & 1].e_, b[2].e_, acc[2], 0, 0, 0);
#define PJ_ROWS3(e_)                                                                                 \
  rem[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(rvq[ks & 1].e_, b[0].e_, rem[0], 0, 0, 0);              \
  rem[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(rvq[ks & 1].e_, b[1].e_, rem[1], 0, 0, 0);              \
  rem[2] = __builtin_amdgcn_mfma_f32_4x4x1f32(rvq[ks & 1].e_, b[2].e_, rem[2], 0, 0, 0);
#define PJ_NO_ROWS(e_)
// The k-loop, fully unrolled so that the ring slots are plain registers (a rotating copy would have to wait for the load it
// copies).  G16_ / G3_: PJ_ROWS16 / PJ_ROWS3 or PJ_NO_ROWS; the statements behind them load the next k-step's A operands
// (avq / rvq[(ks + 1) & 1]).  The prefetches stay in front of the sched_barrier: sunk to just before their use, the LDS reads
// cost ~130 cycles per k-step.
#define PJ_KLOOP(DEPTH_, G16_, G3_, ...)                                                             \
  _Pragma("unroll") for (int ks = 0; ks < 40; ++ks) {                                                \
    if (ks + DEPTH_ - 1 < 40) {                                                                      \
      PJ_W_KSTEP(wk, ks + DEPTH_ - 1)                                                                \
      _Pragma("unroll") for (int n = 0; n < 3; ++n) bq[(ks + DEPTH_ - 1) % DEPTH_][n] = PJ_W_LD(wk, n); \
    }                                                                                                \
    if (ks + 1 < 40) { __VA_ARGS__ }                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                               \
    const float4 *b = bq[ks % DEPTH_];                                                               \
    G16_(x) G3_(x) G16_(y) G3_(y) G16_(z) G3_(z) G16_(w) G3_(w)                                      \
    __builtin_amdgcn_sched_barrier(0);                                                               \
  }
// The 3-row tile's epilogue for one column: the four k sub-steps of a column sit in lanes col, col + 16, col + 32, col + 48 and
// meet in two cross-lane adds; in lane group kk == 0 the statements behind bv_ store row i's value v (bias added).  (As a
// function template with the stores as a callable it moved crnn_stream_kernel's epilogue: EXPERIMENTS 13.)
#define PJ_REM_ROWS(rem_, bv_, ...)                                                                  \
  _Pragma("unroll") for (int i = 0; i < 3; ++i) {                                                    \
    float s3 = rem_[i];                                                                              \
    s3 += __shfl_xor(s3, 16);                                                                        \
    s3 += __shfl_xor(s3, 32);                                                                        \
    if (kk == 0) {                                                                                   \
      const float v = s3 + bv_;                                                                      \
      __VA_ARGS__                                                                                    \
    }                                                                                                \
  }

// ------------------------------------------------------------------------------------------
// crnn_fused_kernel: the whole CRNN for one window in one 4-wave workgroup - the conv output (feat, 48.6 KB per
// window) and the layer-1 input projections (gx1, 14.6 KB) never leave the CU.
//
//   A  stage the 151x40 window transposed into LDS (as conv5x20_kernel)
//   B  conv as implicit GEMM on v_mfma_f32_16x16x4_f32, 6 of the 24 m-tiles per wave -> feat[19][640] in LDS
//   C  layer-1 input projection gx1[19][192] = feat x Wx1^T: the 19 rows are ONE 16-row MFMA tile plus a 3-row
//      remainder on v_mfma_f32_4x4x1_16b_f32 (16 blocks of 4x4x1 at the same 32 MAC/cycle): with the blocks dealt
//      as (k sub-step kk, column quad cg) the B operand is the SAME register as the 16x16x4's
//      (lane = kk*16 + col), the A operand is feat[16 + lane%4][k + 4 kk ..], and the four kk partial sums of a
//      column meet in two cross-lane adds at the very end - 20 rows of matrix time for 19 instead of 32.
//      Each wave owns 3 of the 12 n-tiles over the whole K.  W_x1 (491 KB) streams from L2 straight into registers
//      in B-operand order ([k/4][192][4], one contiguous KB per wave load), three k-steps ahead of its use, addressed as a
//      scalar k-step base + one 32-bit lane offset + the n-tile as the load's immediate (PJ_W_KSTEP): between the projection's
//      960 MFMAs a wave issues its loads and LDS reads and no vector ALU instruction.
//   D  layer-1 recurrence (wave 0 forward, wave 1 backward); every wave's W_x2 operands (B-operand order) on their way
//      from L2 into registers
//   E  layer-2 input projection, the same 16 + 3 row split, A operand out of LDS
//   F  layer-2 recurrence (waves 2, 3) | waves 0, 1 stage the detect head in the dead feat space
//   G  detect head (wave 0)
//
// One wave per SIMD: v_mfma_f32_16x16x4_f32 reaches its issue rate from a single wave with independent accumulators,
// while two such waves on a SIMD got in each other's way (8-wave form of this kernel: the older wave of a SIMD took
// 14.8k cycles over 9.6k cycles of MFMAs and its partner advanced only once it was alone).
// LDS: the window image (28.9 KB; after B it holds the last six feat rows, then gx, seq1, h, the head's small vectors) + feat
// rows 0..12 (33.7 KB; after C the head's first layer) = 62.6 KB (78.1 KB until the end of round 4: CF_FUSED_SMEM_BYTES below),
// two workgroups per CU - one's recurrences and staging run beside the other's MFMA phases - with room for four front-end
// waves beside them (one four-wave workgroup of logmel_rows_kernel, 36,864 B; two two-wave ones of 17 KB until EXPERIMENTS 24).
// ------------------------------------------------------------------------------------------
#define CF_THREADS 256
#define CF_FLD 648  // feat row: 640 + 8; FLD/4 = 162 = 2 (mod 16): the 16-lane groups of the A-operand ds_read_b128 hit 16 distinct slots
#define CF_IMG_FLOATS (CV_ROWS * CV_LDT)
#define CF_FEAT_FLOATS (CV_OT * CF_FLD)
#define CF_SMEM_BYTES ((CF_IMG_FLOATS + CF_FEAT_FLOATS) * 4)
// crnn_fused_kernel keeps only rows 0..12 of feat in the feat region.  Once every wave has read its last image operand the image
// is dead, and the rows the conv produces last go into it as a flat array UNDER gx (which is written last) and clear of seq1 / h
// (which are zeroed first): rows 13..15 as three ordinary feat rows (pitch CF_FLD: the projection's main-tile operand pointer
// advances by the same 16 floats per k-step in every lane, only its base differs), rows 16..18 - the 3-row remainder tile, read
// through a pointer of its own - as a [20][2 k-steps x 3 rows x 16] block behind them (compile-time offsets).
// 78.1 -> 62.6 KB per workgroup: two of them leave two front-end workgroups' 2 x 17 KB free on the CU (timing probes with fewer
// feat rows, same instruction stream: pipelined step 44.7 us at 19 rows, 43.6 at 16, 43.2 at 13, 42.9 at 8: DESIGN.md 7.1).
#define CF_NO_ROW (-0x40000000)                // store offset of a conv row past the window's last one
#define CF_FUSED_FEAT_ROWS 13
#define CF_FUSED_SMEM_BYTES ((CF_IMG_FLOATS + CF_FUSED_FEAT_ROWS * CF_FLD) * 4)
#define CF_ALIAS_ROWS0 24                      // image offset (floats) of feat rows 13..15: (24 - CF_IMG_FLOATS) / 4 = 10 - 2 * 13 (mod 16), i.e. row j
                                               // sits on the 16-byte slot 2 j (mod 16) of the bank cycle like the rows in the feat region
#define CF_ALIAS_REM (CF_ALIAS_ROWS0 + 3 * CF_FLD)  // ... of the remainder block [20][96]
static_assert((((CF_ALIAS_ROWS0 - CF_IMG_FLOATS) / 4 - 2 * 13) % 16 + 16) % 16 == 0 && CF_IMG_FLOATS % 4 == 0, "aliased rows off their bank slots");
static_assert(CV_OT - 16 == 3 && 16 - CF_FUSED_FEAT_ROWS == 3 && CF_ALIAS_REM + 20 * 96 <= 20 * GR_GX_LD /* = CF_SEQ */,
              "the aliased rows must lie under gx");
// offsets (floats) inside the image region once the conv is done
#define CF_GX 0
#define CF_SEQ (20 * GR_GX_LD)
#define CF_HB (CF_SEQ + 32 * GR_SEQ_LD)   // h[layer 2][dir 2][ping-pong 2][32]
#define CF_ENC (CF_HB + 2 * 2 * 2 * GR_H)
#define CF_HID (CF_ENC + 2 * GR_H)
#define CF_W2S (CF_HID + 2 * GR_H)
static_assert(CF_W2S + 8 * 64 <= CF_IMG_FLOATS, "post-conv LDS layout exceeds the image region");
static_assert(64 * GR_W1_LD <= CF_FEAT_FLOATS && 16 * 192 * 4 <= CF_FEAT_FLOATS, "feat region too small for its later tenants");
static_assert(64 * GR_W1_LD <= CF_FUSED_FEAT_ROWS * CF_FLD, "fused kernel's feat region too small for the head's first layer");

struct fused_args {
  const float *mel;
  win_addr wa;
  const float *w4;    // conv weights [CV_KPAD/4][32][4]
  const float *cbias; // [32]
  const float *wx1s;  // W_x1 in B-operand order [640/4][192][4]
  const float *bx1;   // [192]
  const float *wh1, *bh1;
  const float *wx2s;  // W_x2 in B-operand order [64/4][192][4]
  const float *bx2, *wh2, *bh2, *w1, *b1, *w2, *b2;
  float *enc;         // optional [Nw][64]
  float *out;         // [Nw][NOUT]
  int T, NOUT, HEAD;
  long long *stamps;  // crnn_fused_kernel<front>'s phase stamps: [blocks][4 waves][10] s_memtime (nullptr = off; no launch sets it)
  float *gx_out;      // FRONT_ONLY: [Nw][OT][192] layer-1 input projections incl. b_x
  const unsigned short *cwb;   // bf16x3: conv weights, A-operand order [plane 2][k-step 4][m-tile 2][lane 64][8]
  const unsigned short *wx1b;  // bf16x3: W_x1, B-operand order [plane 2][k-step 20][n-tile 12][lane 64][8]
  ww_tick_tag tag;             // streaming ticks: the posterior as a {value, tick number} pair instead of the row of `out` (common.h)
};

// one direction of one GRU layer over the OT steps held in LDS (gx rows incl. b_x), h ping-pong in hd.
// dir is WAVE-UNIFORM and the caller hands it over in a scalar register (wave_index()): the time position is then scalar too,
// and a step's LDS addresses are per-lane pointers formed here, in front of the loop, that move on by a scalar stride (gx row,
// seq1 row) or take the ping-pong slot as an immediate offset (h) - no multiply, no select and no 64-bit arithmetic in a step.
// The loop runs over the two-step period of the h ping-pong, so that the slot is a constant of each copy of the step and the
// values carried from step to step (h_own, the prefetched inputs) change names instead of registers; OT is odd, its last step
// is the tail and has nothing left to fetch ahead.
template <bool SEQ>
__device__ __forceinline__ float cf_recurrence(const gru_w &g, const float *gxs, float *hd, float *seq1, int dir, int unit, int half) {
  constexpr int H = GR_H, OT = CV_OT;
  static_assert(OT % 2 == 1, "the step loop is pairs of steps plus one");
  const int t0 = dir ? OT - 1 : 0;
  const int gx_step = dir ? -GR_GX_LD : GR_GX_LD, seq_step = dir ? -GR_SEQ_LD : GR_SEQ_LD;
  const float *gxp = gxs + t0 * GR_GX_LD + dir * 3 * H + unit;        // this step's projected inputs
  float *sqp = SEQ ? seq1 + t0 * GR_SEQ_LD + dir * H + unit : nullptr; // this step's row of seq1
  float *hw = hd + unit;
  float h_own = 0.f;
  // a step's projected inputs start two of its chains, so they are fetched a step ahead (behind the h reads, which are the
  // ones the step waits for)
  float gz = gxp[0], gr = gxp[H], gc = gxp[2 * H];
#pragma unroll 1
  for (int s = 0; s < OT / 2; ++s) {
    float nz, nr, nc;
    gxp += gx_step;
    h_own = gru_step<true>(g, hd, half, gz, gr, gc, h_own, gxp, nz, nr, nc);
    if (half == 0) {
      hw[H] = h_own;
      if (SEQ) *sqp = h_own;
    }
    if (SEQ) sqp += seq_step;
    wsync_h();
    gxp += gx_step;
    h_own = gru_step<true>(g, hd + H, half, nz, nr, nc, h_own, gxp, gz, gr, gc);
    if (half == 0) {
      hw[0] = h_own;
      if (SEQ) *sqp = h_own;
    }
    if (SEQ) sqp += seq_step;
    wsync_h();
  }
  float nz, nr, nc;  // (not fetched)
  h_own = gru_step<false>(g, hd, half, gz, gr, gc, h_own, nullptr, nz, nr, nc);
  if (half == 0) {
    hw[H] = h_own;
    if (SEQ) *sqp = h_own;
  }
  wsync_h();
  return h_own;
}

// one operand quad of the layer-2 projection: 3 n-tiles x (rows 0..15, rows 16..18), both on 16x16x4 tiles - unlike layer 1's
// PJ_ROWS3, rows 16..18 are a second full tile (its other thirteen rows read zeros), so that ALL nineteen rows are one fmaf
// chain in the same k order - the association gru_tail16_kernel reproduces step by step
#define CF_ROUND_L2(av_, rv_, b_, e_)                                                                  \
  acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.e_, b_[0].e_, acc[0], 0, 0, 0);                     \
  acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.e_, b_[1].e_, acc[1], 0, 0, 0);                     \
  acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av_.e_, b_[2].e_, acc[2], 0, 0, 0);                     \
  rem[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(rv_.e_, b_[0].e_, rem[0], 0, 0, 0);                     \
  rem[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(rv_.e_, b_[1].e_, rem[1], 0, 0, 0);                     \
  rem[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(rv_.e_, b_[2].e_, rem[2], 0, 0, 0);

// Phase E, the layer-2 input projection gx2[t][n] = seq1[t][:] . Wx2[n][:] + bx2[n]  (19 rows, K = 64, N = 192), for the three
// n-tiles nt0 .. nt0 + 2 of a wave: rows 0..15 as one MFMA tile, rows 16..18 as a second one whose lane j reads row rrow of
// seq1 - the caller's choice of a row that is 16 + j for j < 3 and all zeros otherwise.  Every row is the same fmaf chain from
// zero: k = 16 kb + 4 kk + e in the order kb, e, kk, the bias added last.  cf_phases_d_to_g (4 waves x 3 n-tiles, operands
// requested before the recurrence) and gru_tail_kernel (2 waves x 2 passes x 3 n-tiles) run it.
// (Macros: as functions they moved instructions in six kernels, profiles/EXPERIMENTS.md 13.  seq1, gxs, j and kk are the
// kernel's names.)
// W_x2 in B-operand order [64/4][192][4]: 12 x 16 bytes per lane, L2
#define L2_LOAD_W(bq_, wx2s_, nt0_)                                                                  \
  _Pragma("unroll") for (int kb = 0; kb < 4; ++kb)                                                   \
    _Pragma("unroll") for (int n = 0; n < 3; ++n)                                                    \
      bq_[kb][n] = *(const float4 *)((wx2s_) + ((size_t)(kb * 4 + kk) * 192 + ((nt0_) + n) * 16 + j) * 4);
// the biases: requested in front of the products they are added to (asked for where they are used, each of the three was a
// round trip to L2 of its own at the end of the phase)
#define L2_LOAD_BIAS(bb_, bx2_, nt0_) \
  _Pragma("unroll") for (int n = 0; n < 3; ++n) bb_[n] = (bx2_)[((nt0_) + n) * 16 + j];
// the products; the statements behind nt0_ (gru_tail_kernel's barrier: gx2 takes gx1's place); the stores of the 19 rows
#define L2_PROJECT(bq_, bb_, rrow_, nt0_, ...)                                                       \
  {                                                                                                  \
    f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};               \
    f32x4 rem[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};               \
    _Pragma("unroll") for (int kb = 0; kb < 4; ++kb) {                                               \
      const float4 av = *(const float4 *)(&seq1[j * GR_SEQ_LD + kb * 16 + kk * 4]);                  \
      const float4 rv = *(const float4 *)(&seq1[(rrow_) * GR_SEQ_LD + kb * 16 + kk * 4]);            \
      const float4 *b = bq_[kb];                                                                     \
      CF_ROUND_L2(av, rv, b, x) CF_ROUND_L2(av, rv, b, y) CF_ROUND_L2(av, rv, b, z) CF_ROUND_L2(av, rv, b, w) \
    }                                                                                                \
    __VA_ARGS__                                                                                      \
    _Pragma("unroll") for (int n = 0; n < 3; ++n) {                                                  \
      const int col = ((nt0_) + n) * 16 + j;                                                         \
      const float bb = bb_[n];                                                                       \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) gxs[(kk * 4 + r) * GR_GX_LD + col] = acc[n][r] + bb; \
      if (kk == 0) {                                                                                 \
        _Pragma("unroll") for (int r = 0; r < 3; ++r) gxs[(16 + r) * GR_GX_LD + col] = rem[n][r] + bb; \
      }                                                                                              \
    }                                                                                                \
  }

// Phases D..G of the fused kernels (fp32 and split-bf16 front halves share them): gx1 is in LDS, g holds this wave's
// recurrent weights (waves 0, 1: layer 1; waves 2, 3: layer 2).
__device__ __forceinline__ void cf_phases_d_to_g(const fused_args &a, float *img, float *feat, const gru_w &g, int w) {
  constexpr int H = GR_H;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_index(tid);  // (scalar: so are dir and the forks on wave below)
  const int j = lane & 15, kk = lane >> 4;
  const int unit = lane >> 1, half = lane & 1, dir = wave & 1;
  float *gxs = img + CF_GX, *seq1 = img + CF_SEQ, *hb = img + CF_HB, *encs = img + CF_ENC, *hid = img + CF_HID, *w2s = img + CF_W2S;
  // ---- D: layer-1 recurrence (waves 0, 1).  Every wave first requests its B operands of the layer-2 projection (W_x2 in
  //      B-operand order, 12 x 16 bytes per lane, L2): they arrive during the recurrence, and phase E reads nothing but
  //      its A operand from LDS (W_x2 used to be staged through the feat space by waves 2, 3; phase E 4.3 k -> 4.0 k cycles for 1.9 k of MFMAs)
  float4 bq2[4][3];
  L2_LOAD_W(bq2, a.wx2s, wave * 3)
  if (wave < 2) {
    __builtin_amdgcn_s_setprio(3);  // the serial chain issues ahead of a co-resident workgroup's MFMA stream (+1.5 % at scale)
    cf_recurrence<true>(g, gxs, hb + dir * 2 * H, seq1, dir, unit, half);
    __builtin_amdgcn_s_setprio(0);
  }
  __syncthreads();

  // ---- E: layer-2 input projection (L2_PROJECT), 3 n-tiles per wave; rows 19..31 of seq1 are zeros
  {
    float bb2[3];
    L2_LOAD_BIAS(bb2, a.bx2, wave * 3)
    __builtin_amdgcn_sched_barrier(0);
    L2_PROJECT(bq2, bb2, 16 + j, wave * 3, )
  }
  __syncthreads();

  // ---- F: layer-2 recurrence (waves 2, 3): only the last state of each direction is kept | waves 0, 1: head -> LDS
  float *w1s = feat;  // [64][GR_W1_LD]
  if (wave >= 2) {
    __builtin_amdgcn_s_setprio(3);  // the serial chain issues ahead of a co-resident workgroup's MFMA stream (+1.5 % at scale)
    const float h_last = cf_recurrence<false>(g, gxs, hb + (2 + dir) * 2 * H, nullptr, dir, unit, half);
    __builtin_amdgcn_s_setprio(0);
    if (half == 0) {
      encs[dir * H + unit] = h_last;
      if (a.enc) a.enc[(size_t)w * 2 * H + dir * H + unit] = h_last;
    }
  } else {
    for (int i = tid; i < 64 * 64; i += 128) w1s[(i >> 6) * GR_W1_LD + (i & 63)] = a.w1[i];
    for (int i = tid; i < a.NOUT * 64; i += 128) w2s[i] = a.w2[i];
  }
  __syncthreads();

  // ---- G: detect head: Dense(64, relu) -> Dense(NOUT) -> sigmoid | softmax   (wave 0)
  if (wave == 0) {
    const float b1v = a.b1[lane], b2v = a.b2[lane < a.NOUT ? lane : 0];  // on their way during the dot products
    __builtin_amdgcn_sched_barrier(0);
    float acc = 0.f;
#pragma unroll 16
    for (int k = 0; k < 2 * H; ++k) acc = fmaf(w1s[lane * GR_W1_LD + k], encs[k], acc);
    hid[lane] = fmaxf(acc + b1v, 0.f);
    wsync_g();
    float y = 0.f;
    if (lane < a.NOUT) {
      for (int k = 0; k < 2 * H; ++k) y = fmaf(w2s[lane * 64 + k], hid[k], y);
      y += b2v;
    }
    const float p = head_activation(y, lane, a.NOUT, a.HEAD);
    if (a.tag.slots) {
      if (lane == a.tag.pidx) tick_tag_store(a.tag, w, p);
    } else if (lane < a.NOUT) {
      a.out[(size_t)w * a.NOUT + lane] = p;
    }
  }
}

// ---- the CTC head (WW_HEAD_CTC): ONE definition for gru_tail_ctc_kernel and cf_phases_d_to_g_ctc --------------------------------
// One dense layer on every row of layer 2's step outputs, z[t][c] = b2[c] + sum_k w2[c][k] seq2[t][k], then the softmax over the L
// classes of a row.  The 19 x 8 (row, class slot) pairs are dealt over the threads that are free, eight adjacent lanes per row - the
// arrangement head_activation's softmax exchanges in.
// The head's weights [L <= 8][64] as 128 x 16 bytes: thread tid < 128 loads row tid / 16 (rows L..7: zeros) ...
__device__ __forceinline__ float4 ctc_head_w_load(const float *w2, int tid, int L) {
  return tid * 4 < L * 2 * GR_H ? ((const float4 *)w2)[tid] : make_float4(0.f, 0.f, 0.f, 0.f);
}
// ... and parks it in LDS, rows GR_SEQ_LD apart (eight rows 64 apart would share their banks)
__device__ __forceinline__ void ctc_head_w_park(float *w2s, int tid, const float4 w2q) {
  *(float4 *)(&w2s[(tid >> 4) * GR_SEQ_LD + (tid & 15) * 4]) = w2q;
}
// Slot p is (row p / 8, class p % 8); slots past row 18 recompute row 18 and store nothing (every lane of a wave takes part in the
// softmax's exchanges).  One fmaf chain in k order from zero, the bias added last - the association of the other heads' last layer
// (cf_phases_d_to_g, gru_tail_kernel, crnn_detect_kernel) - then head_activation's softmax.  The posterior goes to post[row][8] (LDS)
// and, where steps_w is given, to the window's [19][L] block of the caller's posteriors.
__device__ __forceinline__ void ctc_head_slot(const float *w2s, const float *seq2, float b2v, int p, int L, float *post, float *steps_w) {
  constexpr int OT = CV_OT;
  const int o = p & 7, t = min(p >> 3, OT - 1);
  const float4 *wr = (const float4 *)(w2s + o * GR_SEQ_LD);  // (rows L..7 are zeros)
  float y = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float4 wv = wr[q];
    const float4 sv = *(const float4 *)(&seq2[t * GR_SEQ_LD + q * 4]);
    y = fmaf(wv.x, sv.x, y); y = fmaf(wv.y, sv.y, y);
    y = fmaf(wv.z, sv.z, y); y = fmaf(wv.w, sv.w, y);
  }
  y += b2v;
  const float pr = head_activation(y, o, L, 1 /* softmax */);
  if (o < L && (p >> 3) < OT) {
    post[t * 8 + o] = pr;
    if (steps_w) steps_w[t * L + o] = pr;
  }
}

// Phases D..G of the streaming kernel for a CTC-trained CRNN (crnn_stream_kernel<FE, false, false, CTC>): cf_phases_d_to_g with
// gru_tail_ctc_kernel's back end.  Layer 1 and phase E run through the same macros on the same wave split; layer 2 keeps every step
// (cf_recurrence<true>) in seq2, the head is the shared one above on the three waves it needs, and thread 0 decodes the rows as
// written (ctc_decode.h) and sends the decode out as ONE 32-bit word (stream_ctc.h): the value half of the window's tag where the
// launch has tag slots, else row w of the launch's output block.
// No LDS of its own: seq2, the posterior rows and the head's weights live in the feat region, which is dead behind "gx complete" -
// where the other heads keep w1s, and a CTC model has no w1.
#define CFC_SEQ2 0                                 // floats from `feat`: [19][GR_SEQ_LD], row t = [h_fwd(t) | h_bwd(t)]
#define CFC_POST (CFC_SEQ2 + CV_OT * GR_SEQ_LD)    // [19][8] posteriors
#define CFC_W2S (CFC_POST + CV_OT * 8)             // [8][GR_SEQ_LD] the head's weights
#define CFC_FLOATS (CFC_W2S + 8 * GR_SEQ_LD)
static_assert(CV_OT == WW_SC_STEPS && CFC_SEQ2 % 4 == 0 && CFC_POST % 4 == 0 && CFC_W2S % 4 == 0,
              "cf_phases_d_to_g_ctc's LDS layout is written for 19 steps, 16-byte aligned rows");
static_assert(CFC_FLOATS <= CF_FEAT_FLOATS, "the CTC back end does not fit the feat region");
static_assert(CV_OT * 8 <= 3 * 64, "the head's (row, class slot) pairs are one pass of three waves");
__device__ __forceinline__ void cf_phases_d_to_g_ctc(const fused_args &a, float *img, float *feat, const gru_w &g, int w, float *steps) {
  constexpr int H = GR_H, OT = CV_OT;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_index(tid);  // (scalar: so are dir and the forks on wave below)
  const int j = lane & 15, kk = lane >> 4;
  const int unit = lane >> 1, half = lane & 1, dir = wave & 1;
  float *gxs = img + CF_GX, *seq1 = img + CF_SEQ, *hb = img + CF_HB;
  float *seq2 = feat + CFC_SEQ2, *post = feat + CFC_POST, *w2s = feat + CFC_W2S;
  // ---- D: layer-1 recurrence (waves 0, 1), every wave's W_x2 operands on their way (as cf_phases_d_to_g)
  float4 bq2[4][3];
  L2_LOAD_W(bq2, a.wx2s, wave * 3)
  if (wave < 2) {
    __builtin_amdgcn_s_setprio(3);
    cf_recurrence<true>(g, gxs, hb + dir * 2 * H, seq1, dir, unit, half);
    __builtin_amdgcn_s_setprio(0);
  }
  __syncthreads();

  // ---- E: layer-2 input projection (L2_PROJECT), 3 n-tiles per wave; rows 19..31 of seq1 are zeros
  {
    float bb2[3];
    L2_LOAD_BIAS(bb2, a.bx2, wave * 3)
    __builtin_amdgcn_sched_barrier(0);
    L2_PROJECT(bq2, bb2, 16 + j, wave * 3, )
  }
  __syncthreads();

  // ---- F: layer-2 recurrence (waves 2, 3), every step kept: each (row, direction half) of seq2 is written exactly once, so seq2
  //      needs no clearing | waves 0, 1: the head's weights -> LDS
  const float b2v = a.b2[(tid & 7) < a.NOUT ? (tid & 7) : 0];  // (on its way during the recurrence)
  if (wave >= 2) {
    __builtin_amdgcn_s_setprio(3);
    cf_recurrence<true>(g, gxs, hb + (2 + dir) * 2 * H, seq2, dir, unit, half);
    __builtin_amdgcn_s_setprio(0);
  } else {
    ctc_head_w_park(w2s, tid, ctc_head_w_load(a.w2, tid, a.NOUT));
  }
  __syncthreads();

  // ---- G: the head: 19 x 8 slots on waves 0..2, one pass
  if (wave < 3) {
    ctc_head_slot(w2s, seq2, b2v, tid, a.NOUT, post, steps ? steps + (size_t)w * OT * a.NOUT : nullptr);
  }
  __syncthreads();
  // greedy decode of the posteriors as written, packed
  if (tid == 0) {
    int32_t *lab = (int32_t *)w2s;  // (the head is through with its weights)
    const int32_t len = ww_ctc_greedy_row(post, OT, a.NOUT, 8, lab, WW_STREAM_CTC_MAX_LABELS);
    const unsigned word = ww_sc_pack(lab, len);
    if (a.tag.slots) tick_tag_store(a.tag, w, word);
    else ((unsigned *)a.out)[w] = word;  // (the launch's output block holds words, not floats)
  }
}

// crnn_fused_kernel<front> alone keeps its stamp sites: without them its compiled form ran ~1 % slower at 16,384 windows
// per launch (the other forms lost theirs at no cost; profiles/EXPERIMENTS.md 9.5)
#define CF_STAMP(i_) \
  if (FRONT_ONLY && a.stamps && lane == 0) a.stamps[((size_t)blockIdx.x * 4 + wave) * 10 + (i_)] = __builtin_amdgcn_s_memtime();
// SET (a model set's batch, ww_k_crnn_forward with a set): window blockIdx.x is evaluated by member set.ids[blockIdx.x] - the weight
// pointers move on to that member's block before anything is read through them, and from there on the kernel is the
// single-model kernel, instruction for instruction.
__device__ __forceinline__ void cf_set_move(fused_args &a, long long off) {
  ww_set_move(a.w4, off); ww_set_move(a.cbias, off); ww_set_move(a.wx1s, off); ww_set_move(a.bx1, off);
  ww_set_move(a.wh1, off); ww_set_move(a.bh1, off); ww_set_move(a.wx2s, off); ww_set_move(a.bx2, off);
  ww_set_move(a.wh2, off); ww_set_move(a.bh2, off); ww_set_move(a.w1, off); ww_set_move(a.b1, off);
  ww_set_move(a.w2, off); ww_set_move(a.b2, off); ww_set_move(a.cwb, off); ww_set_move(a.wx1b, off);
}
template <bool FRONT_ONLY, bool SET = false>
__global__ __launch_bounds__(CF_THREADS, 2) void crnn_fused_kernel(fused_args a, ww_set_ref set) {
  if constexpr (SET) cf_set_move(a, ww_set_offset(set, blockIdx.x));
  extern __shared__ __align__(16) float cf_smem[];
  float *img = cf_smem, *feat = cf_smem + CF_IMG_FLOATS;
  constexpr int H = GR_H, OT = CV_OT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kk = lane >> 4;
  const int w = blockIdx.x;
  CF_STAMP(0)
  int64_t row;
  int valid;
  window_span(a.wa, w, a.T, row, valid);

  // conv weights for this lane (B operand of mfma 16x16x4: lane (j, kk)); issued first, used after the staging
  float4 wreg[CV_KB][2];
  float wlast[2], cb0, cb1;
  CV_LOAD_W(wreg, wlast, cb0, cb1, a.w4, a.cbias)

  // ---- A: stage the window (loads first, then zero the image, then the transposed scatter)
  int a_off[6], o_off[6][4];
  {
    constexpr int MAXV = 6;  // 6 * 256 float4 >= 151 * 40 / 4
    const float *src = a.mel + row * CV_NMEL;
    const int n = valid * CV_NMEL;
    const bool al16 = ((((uintptr_t)src) & 15) == 0);
    float4 stage[MAXV];
    // n is a multiple of 4: a float4 is inside the window or outside it.  Outside ones are never scattered, so they load the
    // window's last float4 again instead of being masked: six unconditional loads, all in flight at once
    if (n > 0)
      stage_loads(al16, [&](auto al) {
        constexpr bool AL = decltype(al)::value;
#pragma unroll
        for (int q = 0; q < MAXV; ++q) {
          const int i = (q * CF_THREADS + tid) * 4;
          stage[q] = ld_mel4<AL>(src + (i < n ? i : n - 4), true);
        }
      });
    LDS_CLEAR16(img, CF_IMG_FLOATS / 4, CF_THREADS)
    // while the window is on its way: LDS offsets of this lane's conv operands and results for its six m-tiles
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      constexpr int M = CV_OT * CV_OF;
      const int mt = wave + 4 * i;
      int m = mt * 16 + j;
      if (m >= M) m = M - 1;
      const int t = m / CV_OF, f = m - t * CV_OF;
      a_off[i] = (f * CV_SF) * CV_LDT + t * CV_ST;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int mo = mt * 16 + kk * 4 + r;
        const int to = mo / CV_OF, fo = mo - to * CV_OF;
        // offsets from `feat`; rows 13..15 (in tiles 4) and 16..18 (tiles 5) go into the image, below feat: negative offsets.
        // remainder block: k = 32 fo + 16 n + j is k-step 2 fo + n -> row fo of the block, column 48 n + 16 (t - 16) + j
        // (i is a compile-time constant: tiles 0..3 hold rows t <= 12, tile 4 rows 12..15, tile 5 rows 16..18 and, in wave 3, rows past M)
        if (i < 4) o_off[i][r] = to * CF_FLD + fo * 32 + j;
        else if (i == 4) o_off[i][r] = (to < 13 ? to * CF_FLD : CF_ALIAS_ROWS0 - CF_IMG_FLOATS + (to - 13) * CF_FLD) + fo * 32 + j;
        else o_off[i][r] = mo >= M ? CF_NO_ROW : CF_ALIAS_REM - CF_IMG_FLOATS + fo * 96 + 16 * (to - 16) + j;
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MAXV; ++q) {
      const int i = (q * CF_THREADS + tid) * 4;
      if (i < n) {  // the four features are four consecutive mel bins of ONE frame (40 = 10 x 4): one division, four rows of the image
        const int it = i / CV_NMEL, im = i - it * CV_NMEL;
        float *d = img + (im + CV_PF) * CV_LDT + it + CV_PT;
        d[0] = stage[q].x;
        d[CV_LDT] = stage[q].y;
        d[2 * CV_LDT] = stage[q].z;
        d[3 * CV_LDT] = stage[q].w;
      }
    }
  }
  __syncthreads();
  CF_STAMP(1)
  PJ_W_LANE(a.wx1s)
  float4 bq[4][3];
  // ---- B: conv -> feat (LDS).  Six m-tiles per wave (CV_TILE_LOOP), operand and store offsets from the staging (a_off, o_off)
  {
    auto load_a = [&](cv_a &av, int i) { CV_LOAD_A(av, img + a_off[i]) };
    auto store_tile = [&](int i, const f32x4 &r0, const f32x4 &r1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (i < 5) {
          feat[o_off[i][r]] = relu1(r0[r]);
          feat[o_off[i][r] + 16] = relu1(r1[r]);
        } else if (o_off[i][r] != CF_NO_ROW) {  // (only the last tile of wave 3 has rows past M); the remainder block's channel halves are 48 apart
          feat[o_off[i][r]] = relu1(r0[r]);
          feat[o_off[i][r] + 48] = relu1(r1[r]);
        }
      }
    };
    f32x4 prev0 = {0.f, 0.f, 0.f, 0.f}, prev1 = {0.f, 0.f, 0.f, 0.f}, t4_0 = prev0, t4_1 = prev0;
    // tiles 4 and 5 hold the rows that go into the image: kept until it is dead
    CV_TILE_LOOP(6, if (i > 0 && i < 5) store_tile(i - 1, prev0, prev1); if (i == 5) { t4_0 = prev0; t4_1 = prev1; })
    // the projection's first W operands: requested here, in front of the two barriers (they do not wait for global loads)
    PJ_RING_PROLOGUE(4)
    __builtin_amdgcn_sched_barrier(0);
    lds_barrier();  // every wave has read its last image operand: rows 13..18 of feat may take the image's place
    store_tile(4, t4_0, t4_1);
    store_tile(5, prev0, prev1);
  }
  CF_STAMP(2)
  lds_barrier();  // feat complete (rows 0..12 in the feat region, rows 13..18 in the image, which holds nothing else any more)
  CF_STAMP(3)
  float *gxs = img + CF_GX, *seq1 = img + CF_SEQ, *hb = img + CF_HB;
  CLEAR_SEQ_H(seq1, 32, hb, CF_THREADS)  // (behind gx: clear of the aliased rows)

  // ---- C: layer-1 input projection
  const int unit = lane >> 1, half = lane & 1, dir = wave & 1;
  gru_w g;  // waves 0, 1: layer 1; waves 2, 3: layer 2
  {
    const float *a0p = (j < 13 ? feat + j * CF_FLD : img + CF_ALIAS_ROWS0 + (j - 13) * CF_FLD) + kk * 4;  // rows 13..15: in the image
    const int r1 = (lane & 3) < 3 ? (lane & 3) : 2;  // rows 16 + r1; lane % 4 == 3: row 19 does not exist, its sums are never stored
    const float *a1p = img + CF_ALIAS_REM + 16 * r1 + kk * 4;  // the remainder block: k-step ks is its row ks / 2, columns 48 (ks % 2) ..
    f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    f32x4 rem[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    // operand ring: W three k-steps ahead (L2), feat one step ahead (LDS)
    float4 avq[2], rvq[2];
    avq[0] = *(const float4 *)(a0p);
    rvq[0] = *(const float4 *)(a1p);
    float bv1[3];
    PJ_LOAD_BIAS(bv1, a.bx1)
    // recurrent weights: requested here too (48 registers the projection does not need), used a barrier (waves 0, 1) or a whole
    // recurrence (waves 2, 3) later - requested behind the projection they arrived in the first ~800 cycles of phase D
    if (!FRONT_ONLY) gru_load_w(g, wave < 2 ? a.wh1 : a.wh2, wave < 2 ? a.bh1 : a.bh2, dir, unit, half);
    PJ_KLOOP(4, PJ_ROWS16, PJ_ROWS3,
             avq[(ks + 1) & 1] = *(const float4 *)(a0p + (ks + 1) * 16);
             rvq[(ks + 1) & 1] = *(const float4 *)(a1p + ((ks + 1) >> 1) * 96 + ((ks + 1) & 1) * 48);)
    lds_barrier();  // gx takes the aliased block's place: every wave must have read its last remainder operand out of it
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const int col = wave * 48 + n * 16 + j;
      const float bv = bv1[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) gxs[(kk * 4 + r) * GR_GX_LD + col] = acc[n][r] + bv;
      PJ_REM_ROWS(rem[n], bv, gxs[(16 + i) * GR_GX_LD + col] = v;)
    }
  }
  CF_STAMP(4)
  __syncthreads();  // gx complete; nobody reads feat any more
  CF_STAMP(5)
  if (FRONT_ONLY) {
    // large batches: the recurrences run in their own kernel (gru_tail_kernel), where seven windows share a CU and no MFMA
    // stream competes with their serial chains; gx1 (14.6 KB per window) crosses memory instead of feat (48.6 KB)
    float4 *dst = (float4 *)(a.gx_out + (size_t)w * OT * 6 * H);
    for (int q = tid; q < OT * 6 * H / 4; q += CF_THREADS) {
      const int e = q * 4, t = e / (6 * H), c = e - t * 6 * H;
      dst[q] = *(const float4 *)(&gxs[t * GR_GX_LD + c]);
    }
    return;
  }

  cf_phases_d_to_g(a, img, feat, g, w);
}

// ------------------------------------------------------------------------------------------
// crnn_stream_kernel: crnn_fused_kernel for the streaming mode (spokestack/wakeword/tflite.py:187-188: the window slides
// by ONE mel row per posterior).  The conv and the layer-1 input projection act on each of the 19 time positions of a
// window separately, and position t looks at mel rows 8 t - 6 .. 8 t + 13 of the window: positions 1..17 never see the
// window's zero padding, so their projected rows gx1[t] are functions of 20 consecutive mel rows of the STREAM - the row
// that is position 17 of the window ending at stream row r is position 16 of the window ending at r + 8, ... position 1
// at r + 128.  Per stream a ring of WW_STREAM_GXC rows of gx1 (keyed by r mod ring size) keeps them: a new window
// computes THREE positions (0 and 18, which touch the padding, and the new interior one, 17, which it also stores) instead
// of 19, fetches the other sixteen rows (12 KB, L2) and runs the recurrences and the head as crnn_fused_kernel does.
// 1.3 instead of 8.0 MFLOP per posterior; what remains of the kernel's time is the recurrences (phases D..G).
// After a reset every slot holds the row of an all-zero field (the mel history is zeros), which is what the positions
// in front of the stream's first rows must see.  Rows differ from the batch kernel's in the last bits where the batch
// kernel computes a position on the 16-row MFMA tile and this one on the 4x4x1 form (different association of the k sum).
// ------------------------------------------------------------------------------------------
#ifndef CS_DEPTH
#define CS_DEPTH 8
#endif
struct stream_args {
  fused_args f;
  const int32_t *aux;  // [nw] stream * WW_STREAM_GXC + (stream rows incl. this window's newest) % WW_STREAM_GXC
  float *gxc;          // [S][WW_STREAM_GXC][192]
  // FE != 0 - ONE launch per tick: the streaming front end's side and the model's filterbank (stream_fe.h)
  ww_tick_fe fe;
  ww_fe_filt fb;
};

// Mel-side LDS of the one-launch tick form (stream_fe.h: fe_tick_lds), in the part of the feat region the three conv rows leave free
#define CT_BASE (3 * CF_FLD)  // floats from `feat`; the weights go in in three store rounds of 256 x 16 bytes
static_assert(CT_BASE % 4 == 0 && CT_BASE + FE_TL_FLOATS <= CF_FEAT_FLOATS, "tick front end does not fit beside the conv rows");

// FE = 0: the windows of a tick come as descriptor tables behind a front-end kernel of its own (stream_frontend_kernel: two
// launches per tick).  FE = 1 / 2 (fp32 / fp64 transform) - ONE launch per tick (round 5): workgroup 2 s + k is window k of stream
// s's tick and transforms the new frames itself - waves 0 and 1, one frame each, straight into the window image, while the
// other waves stage the rows that were there before; spokestack/wakeword/tflite.py:148-191 for one stream.  Two workgroups of
// one stream run in the same launch, so exactly ONE of them writes the stream's state - the workgroup of the tick's newest
// window (k = n_windows - 1; workgroup 2 s when the tick has no window: the ring still advances, tflite.py:163-168) stores
// both new mel rows, the ring tail and the pre-emphasis carry - and its sibling must still see last tick's: the mel rows it
// reads are not the slots written this tick (the mirrored ring of T + 1 slots leaves exactly those out), the sample ring and
// the carry are kept twice and ping-pong by the stream's state parity.  The sibling transforms frame 0 a second time (same
// instructions, same bits) rather than wait for it.  No kernel boundary, no second launch, no descriptor tables; the
// posteriors go out as {value, tick number} pairs (ww_tick_tag) that the host polls.
// SET (a bank created from a model set): the workgroup's member is set.ids[its stream] - FE != 0: stream blockIdx.x / 2; FE = 0: the
// stream in the window's aux word.
// ALL (FE != 0, SET: a bank that runs K member slots on every stream, stream_all.h): the grid is 2 S K, workgroup w is window
// k = w & 1 of VIRTUAL stream v = w >> 1 = s K + slot.  The model side stays a function of v - the member set.ids[v], v's cache of
// projected rows, tag slot w - and the front-end side reads PHYSICAL stream s = v / K (K: set.K, a kernel argument; s and slot are
// scalars): the frames, the control words, ring[par], prev[par], the mel rows.  A stream now has 2 K workgroups and still exactly
// ONE writer: the newest window's workgroup of slot 0 (fe_tick_decode).  Why the other 2 K - 1 need no order with it, whichever of
// them runs first - a grid above what is resident at once starts siblings after their stream's writer has long finished:
//   * every workgroup reads ring[par] and prev[par], last tick's copies; the writer stores ring[par ^ 1] and prev[par ^ 1] only.
//     The copy a tick reads is written next by the NEXT tick's kernel, which the stream orders behind every workgroup of this one;
//   * window k reads mel slots pos + k + 2 .. pos - 1 (mod T + 1) of the mirrored ring, T - k - 1 rows, and takes the tick's new
//     rows from its own transforms.  The writer stores slots pos and pos + 1 (and their mirrors, T + 1 rows on): never a slot in
//     that range, for k = 0 and k = 1 alike - the one spare slot of the ring;
//   * the control words and frames are host memory that nobody writes during the tick;
//   * what a workgroup writes besides is v's own: cache slot q0 + 128 (read by neither window of v this tick: they read q0 .. q0 +
//     120 of a ring of 144) and tag slot w.
// So no workgroup reads a word that another workgroup of the launch writes, and a sibling that starts late transforms the same
// samples from the same copies: the same instructions on the same values as slot 0's, the same bits as a bank of that member alone.
struct ww_set_all_ref : ww_set_ref {
  int K = 1;  // member slots per stream
};
// CTC: a CTC bank runs one model, so the kernel's second argument is not a set's tables but the launch's posteriors
// [windows][19][L] in page-locked memory (nullptr: not asked for) - stream_args and the other forms' arguments stay as they are
struct ww_ctc_ref {
  float *steps;
};
template <bool ALL, bool CTC>
using cs_second_arg = typename std::conditional<CTC, ww_ctc_ref, typename std::conditional<ALL, ww_set_all_ref, ww_set_ref>::type>::type;
// CTC (a CTC stream bank, streams.hip: ww_stream_create_ctc): everything up to "gx complete" is the kernel as it is; behind it
// cf_phases_d_to_g_ctc keeps layer 2's nineteen steps, runs the per-row softmax head and decodes on the device.
template <int FE, bool SET = false, bool ALL = false, bool CTC = false>
__global__ __launch_bounds__(CF_THREADS, 2) void crnn_stream_kernel(stream_args sa, cs_second_arg<ALL, CTC> set) {
  static_assert(!ALL || (SET && FE != 0), "the every-member form is a one-launch tick of a set bank");
  static_assert(!CTC || (!SET && !ALL), "a CTC bank runs one model: CTC members of model sets are not offered");
  if constexpr (SET && FE != 0) cf_set_move(sa.f, ww_set_offset(set, blockIdx.x >> 1));
  const fused_args &a = sa.f;
  extern __shared__ __align__(16) float cf_smem[];
  float *img = cf_smem, *feat = cf_smem + CF_IMG_FLOATS;
  constexpr int H = GR_H, RA = WW_STREAM_GXC;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kk = lane >> 4;
  const int w = blockIdx.x;
  float4 wreg[CV_KB][2];
  float wlast[2], cb0, cb1;
  float4 crow0, crow1, crow2;
  int a_off, o_off[4];
  int q0;
  float *cache;
  auto load_conv_w = [&]() { CV_LOAD_W(wreg, wlast, cb0, cb1, a.w4, a.cbias) };
  // ---- the sixteen cached rows (positions 1..16): requested first, parked in LDS once the image is dead
  // (three named registers: as an array they stayed in scratch memory)
  auto cached = [&](int q) {
    const int i = tid + q * CF_THREADS, tr = i / 48, c4 = i - tr * 48;  // 16 rows x 48 float4
    int slot = q0 + 8 * tr;
    slot = slot >= RA ? slot - RA : slot;
    return *(const float4 *)(cache + (size_t)slot * (6 * H) + c4 * 4);
  };
  // the three positions as 60 rows (p, f) of ONE m-tile per wave: p = 0, 1, 2 <-> t = 0, 17, 18
  auto tile_offsets = [&]() {
    constexpr int M = 3 * CV_OF;
    int m = wave * 16 + j;
    m = m < M ? m : M - 1;
    const int p = m / CV_OF, f = m - p * CV_OF, t = p ? 16 + p : 0;
    a_off = (f * CV_SF) * CV_LDT + t * CV_ST;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mo = wave * 16 + kk * 4 + r, po = mo / CV_OF, fo = mo - po * CV_OF;
      o_off[r] = mo < M ? po * CF_FLD + fo * 32 + j : -1;
    }
  };
  auto scatter = [&](const float4 (&stage)[2], const int (&sidx)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (sidx[q] >= 0) {
        const int it = sidx[q] / 10, im = (sidx[q] - it * 10) * 4;
        const float e[4] = {stage[q].x, stage[q].y, stage[q].z, stage[q].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) img[(im + c + CV_PF) * CV_LDT + it + CV_PT] = e[c];
      }
    }
  };
  if constexpr (FE == 0) {
    // the window's three descriptor words (first mel row, valid rows, cache slot) in ONE load: lanes 0..3 read the two halves of
    // row[w], valid[w] and aux[w] (three arrays, one instruction), the values come back as scalars - read one after the other they
    // were three round trips in a row at the head of every tick's kernel (the streaming path always passes both tables)
    const int *dp = lane == 0 ? (const int *)(a.wa.row + w) : lane == 1 ? (const int *)(a.wa.row + w) + 1
                  : lane == 2 ? (const int *)(a.wa.valid + w) : (const int *)(sa.aux + w);
    const int dv = *dp;
    int64_t row = (int64_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dv, 1) << 32) | (unsigned)__builtin_amdgcn_readlane(dv, 0));
    int valid = __builtin_amdgcn_readlane(dv, 2);
    const int aux = __builtin_amdgcn_readlane(dv, 3);
    if (valid > a.T) valid = a.T;  // (as window_span)
    if (row + valid > a.wa.mel_rows) valid = (int)(a.wa.mel_rows - row);
    if (valid < 0) valid = 0;
    q0 = aux % RA;
    cache = sa.gxc + (size_t)(aux - q0) * (6 * H);
    if constexpr (SET) cf_set_move(sa.f, ww_set_offset(set, aux / RA));
    load_conv_w();
    crow0 = cached(0); crow1 = cached(1); crow2 = cached(2);
    // ---- A: mel rows 0..13 (position 0) and 130..150 (positions 17, 18) of the window -> the transposed image
    const float *src = a.mel + row * CV_NMEL;  // 160-byte rows of a hipMalloc'ed history: 16-byte aligned
    float4 stage[2];
    int sidx[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int i = tid + q * CF_THREADS;            // 140 + 210 float4
      const int f4 = i < 140 ? i : 1300 + (i - 140);  // float4 index inside the [151][40] window
      const bool in = i < 350 && f4 / 10 < valid;
      sidx[q] = in ? f4 : -1;
      stage[q] = in ? *(const float4 *)(src + (size_t)f4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    LDS_CLEAR16(img, CF_IMG_FLOATS / 4, CF_THREADS)
    tile_offsets();
    __syncthreads();
    scatter(stage, sidx);
  } else {
    typedef typename std::conditional<FE == 2, double, float>::type R;
    const ww_tick_fe &fe = sa.fe;
    const int v = w >> 1, k = w & 1;  // the virtual stream (stream_all.h); an ordinary bank: the stream itself
    int s = v, slot = 0;
    if constexpr (ALL) {
      s = __builtin_amdgcn_readfirstlane((int)((unsigned)v / (unsigned)set.K));
      slot = v - s * set.K;
    }
    // ---- over the bus, together: the tick's 320 samples (40 x 16 bytes) and the stream's control words
    uint4 raw = make_uint4(0u, 0u, 0u, 0u);
    if (tid < 40) raw = ((const uint4 *)(fe.frames + (size_t)s * WW_CHUNK))[tid];
    const int4 cw = ((const int4 *)fe.ctl)[s];
    // ---- device-side inputs that do not depend on the control words, requested while those are crossing the bus: the mel
    // weights, the sample ring (threads 0..127 ask for the copy of parity 0, the others for parity 1: 128 x 4 = 512 > fill),
    // both copies of the carry, the transform's constants (waves 0, 1: one new frame each), the conv weights
    f32x4 wlq[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int i = tid + q * CF_THREADS;
      wlq[q] = ((const f32x4 *)sa.fb.wpad)[i < WW_MEL_TAPS * 64 / 4 ? i : 0];
    }
    const int mel_st = lane < sa.fb.n_mel ? sa.fb.start[lane] : 0;
    const float mel_bias = lane < sa.fb.n_mel ? sa.fb.bias[lane] : 0.0f;
    const float4 ringq = ((const float4 *)(fe.ring + ((size_t)(tid >> 7) * fe.S + s) * WW_ST_RING))[tid & 127];
    const float carry0 = fe.prev[s], carry1 = fe.prev[fe.S + s];
    fft_consts<R> fc;
    if (wave < 2) fft_load_consts<R>(fc, lane, sa.fb.hann, sa.fb.tw256, sa.fb.tw512);
    load_conv_w();
    // ---- what this workgroup is (uniform over it)
    const int slots = a.T + 1;
    const fe_tick_ctl c = fe_tick_decode(cw, k, slots, slot);
    if (c.idle) return;
    float4 stage[2];
    int sidx[2] = {-1, -1};
    if (c.window) {
      q0 = c.rowq + k + 1;  // rows since the reset incl. this window's newest, mod the cache ring
      q0 = q0 >= RA ? q0 - RA : q0;
      cache = sa.gxc + (size_t)v * RA * (6 * H);
      crow0 = cached(0); crow1 = cached(1); crow2 = cached(2);
      const float *src = a.mel + ((size_t)s * fe.HR + c.b) * CV_NMEL;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int i = tid + q * CF_THREADS;            // 140 + 210 float4
        const int f4 = i < 140 ? i : 1300 + (i - 140);  // float4 index inside the [151][40] window
        const bool in = i < 350 && f4 / 10 < a.T - c.nfk;  // (the rows of this tick come from waves 0, 1)
        sidx[q] = in ? f4 : -1;
        stage[q] = in ? *(const float4 *)(src + (size_t)f4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    const fe_tick_lds<R> l = FE_TICK_LDS(R, feat + CT_BASE);
#pragma unroll
    for (int q = 0; q < 3; ++q) ((f32x4 *)l.wl)[tid + q * CF_THREADS] = wlq[q];
    if ((tid >> 7) == c.par) ((float4 *)l.x)[tid & 127] = ringq;
    if (tid < 40) ((uint4 *)l.xs)[tid] = raw;
    if (c.window) {
      LDS_CLEAR16(img, CF_IMG_FLOATS / 4, CF_THREADS)
      tile_offsets();
    }
    __syncthreads();
    // ---- [ring | new samples]: normalise, clip, pre-emphasise
    for (int i = tid; i < WW_CHUNK; i += CF_THREADS) l.x[c.fill + i] = fe_sample(l.xs, i, c.par ? carry1 : carry0, fe.cv);
    __syncthreads();
    // tflite.py:156-158: the carry is the un-emphasised last sample
    if (c.writer && tid == 0) fe.prev[(size_t)(c.par ^ 1) * fe.S + s] = fe_norm(l.xs[WW_CHUNK - 1], fe.cv);
    // ---- new frames: wave f transforms frame f, its mel row goes straight into the window image (time T - nfk + f) and,
    // from the writer, into the stream's mirrored ring
    if (wave < c.nfk) {
      const float mv = fe_frame_mel<R>(l.x + wave * fe.hop, fc, l.buf, l.mag, wave, l.wl, mel_st, mel_bias, sa.fb, lane);
      if (lane < CV_NMEL) {
        img[(lane + CV_PF) * CV_LDT + (a.T - c.nfk + wave) + CV_PT] = mv;
        if (c.writer) fe_ring_store(fe.hist, (size_t)s * fe.HR, c.pos + wave, slots, CV_NMEL, lane, mv);
      }
    }
    if (c.writer) {  // keep the ring tail (for the next tick: the other copy)
      const int keep = c.fill + WW_CHUNK - c.nf * fe.hop;
      float *ring = fe.ring + ((size_t)(c.par ^ 1) * fe.S + s) * WW_ST_RING;
      for (int i = tid; i < keep; i += CF_THREADS) ring[i] = l.x[c.nf * fe.hop + i];
    }
    if (!c.window) return;  // the tick has no window for this stream: its ring has advanced, that is all
    scatter(stage, sidx);
  }
  __syncthreads();
  // ---- B: conv of the 60 rows -> feat[p][f * 32 + channel]
  {
    cv_a av;
    CV_LOAD_A(av, img + a_off)
    f32x4 acc0 = {cb0, cb0, cb0, cb0}, acc1 = {cb1, cb1, cb1, cb1};
#pragma unroll
    for (int kb = 0; kb < CV_KB; ++kb) { CV_MFMA_KB(av, kb) }
    CV_MFMA_LAST(av)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (o_off[r] >= 0) {
        feat[o_off[r]] = relu1(acc0[r]);
        feat[o_off[r] + 16] = relu1(acc1[r]);
      }
    }
  }
  PJ_W_LANE(a.wx1s)
  // W_x1 ring: with three rows the projection is bound by how many bytes of W are in flight, not by the matrix pipe
  // (3.8 k cycles of MFMAs against 491 KB per workgroup): CS_DEPTH - 1 k-steps ahead instead of the batch kernel's three
  float4 bq[CS_DEPTH][3];
  PJ_RING_PROLOGUE(CS_DEPTH)
  __syncthreads();  // feat complete; the image is dead from here on
  float *gxs = img + CF_GX, *seq1 = img + CF_SEQ, *hb = img + CF_HB;
  CLEAR_SEQ_H(seq1, 32, hb, CF_THREADS)
  auto park = [&](int q, const float4 v) {
    const int i = tid + q * CF_THREADS, tr = i / 48, c4 = i - tr * 48;
    *(float4 *)(&gxs[(tr + 1) * GR_GX_LD + c4 * 4]) = v;
  };
  park(0, crow0); park(1, crow1); park(2, crow2);

  // ---- C: layer-1 input projection of the three rows on v_mfma_f32_4x4x1_16b_f32 (the batch kernel's 3-row remainder form)
  const int unit = lane >> 1, half = lane & 1, dir = wave & 1;
  gru_w g;
  {
    const int r1 = lane & 3;
    const float *a1p = feat + (r1 < 3 ? r1 : 2) * CF_FLD + kk * 4;  // lane % 4 == 3: no fourth row, its sums are never stored
    f32x4 rem[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float4 rvq[2];
    rvq[0] = *(const float4 *)(a1p);
    float bv1[3];
    PJ_LOAD_BIAS(bv1, a.bx1)
    gru_load_w(g, wave < 2 ? a.wh1 : a.wh2, wave < 2 ? a.bh1 : a.bh2, dir, unit, half);  // (as crnn_fused_kernel: in front of the projection)
    PJ_KLOOP(CS_DEPTH, PJ_NO_ROWS, PJ_ROWS3, rvq[(ks + 1) & 1] = *(const float4 *)(a1p + (ks + 1) * 16);)
    int nslot = q0 + 128;
    nslot = nslot >= RA ? nslot - RA : nslot;
    float *crow_new = cache + (size_t)nslot * (6 * H);
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const int col = wave * 48 + n * 16 + j;
      const float bv = bv1[n];
      // rows 0, 17, 18; position 17 is position 16 of the window 8 rows on, ... position 1 of the one 128 on: into the cache too
      PJ_REM_ROWS(rem[n], bv, gxs[(i ? 16 + i : 0) * GR_GX_LD + col] = v; if (i == 1) crow_new[col] = v;)
    }
  }
  __syncthreads();  // gx complete; nobody reads feat any more
  if constexpr (CTC) cf_phases_d_to_g_ctc(a, img, feat, g, w, set.steps);
  else cf_phases_d_to_g(a, img, feat, g, w);
}

// ------------------------------------------------------------------------------------------
// crnn_rows_kernel: conv + layer-1 input projection of SIXTEEN time positions per workgroup, for windows that slide over
// one mel sequence with a regular hop (utils/evaluate_models.py:66-73: hop 2).  Positions 1..17 of a window do not see
// its zero padding, so their projected rows are functions of 20 consecutive rows of the sequence and are shared by
// the windows that lie 8, 16, ... rows further on (crnn_stream_kernel is the one-row-at-a-time form of the same fact):
// per window 1 + 2 instead of 19 positions are computed - the new interior field and the two edge positions 0 and 18,
// which are the same conv with the taps over the padding cleared (conv_wL / conv_wR) applied to the sequence's real rows.
// Three position lists ("kinds"): interior fields at stride g = gcd(hop, 8) rows, left edges and right edges at stride hop.
// A workgroup stages the union of its 16 fields (15 stride + 20 <= 140 rows) once, runs the conv as 20 m-tiles
// (position, frequency) and the projection as ONE full 16-row MFMA tile per n-tile - no 3-row remainder, and W_x1 is
// streamed once per 16 rows that are then used by 16 x 17 / 3 windows.  gru_tail_kernel gathers a window's 19 rows.
// SET (a model set's sliding form, ww_k_crnn_segments_forward with a set's call): a two-dimensional grid - blockIdx.x is the tile as ever,
// blockIdx.y the call's member slot, whose member is set.ids[blockIdx.y].  The weight pointers move on to that member's block,
// and the slot writes plane blockIdx.y of the three lists (planes of set.aux[0] interior fields / set.aux[1] edge rows).  The
// tile table is the geometry's and the hop's: one table for every slot.  From there on it is the single-model kernel.
// ------------------------------------------------------------------------------------------
// A set's sliding launches: what the planes hold, read as scalars through ww_set_ref::aux
#define WW_SLIDE_AUX_NI 0  // interior fields per plane of gI
#define WW_SLIDE_AUX_NW 1  // windows of the group per member: rows per plane of gL / gR, and what the tail16 scratch is sized by
#define WW_SLIDE_AUX_W 2   // windows of the CALL per member: rows per plane of the output
#define WW_SLIDE_AUX_N 4
struct rows_args {
  const float *mel;
  int64_t mel_rows;
  const float *w4[3];  // conv weights per kind: interior, left edge, right edge
  const float *cbias, *wx1s, *bx1;
  float *out[3];       // [count][192] per kind (b_x included)
  int64_t start[3];    // mel row of position 0's field (may lie outside the sequence: rows outside read as zeros)
  int stride[3], count[3], tiles[3];
  const rows_tile *desc;  // or: one descriptor per workgroup (launch_plan.h; several sequences in one buffer: ww_k_crnn_segments_forward)
};

template <bool SET = false>
__global__ __launch_bounds__(CF_THREADS, 2) void crnn_rows_kernel(rows_args a, ww_set_ref set) {
  // (the moved pointers are names of their own, read where the single-model kernel reads its arguments - RK_ARG: a.w4 / a.out are
  // chosen by kind where the kernel arguments lie, and a written-to copy of `a` would have to be indexed in registers or scratch)
  const float *m_cbias = nullptr, *m_wx1s = nullptr, *m_bx1 = nullptr;
  long long set_off = 0;
  if constexpr (SET) {
    set_off = ww_set_offset(set, blockIdx.y);
    m_cbias = a.cbias; m_wx1s = a.wx1s; m_bx1 = a.bx1;
    ww_set_move(m_cbias, set_off); ww_set_move(m_wx1s, set_off); ww_set_move(m_bx1, set_off);
  }
#define RK_ARG(name_) (SET ? m_##name_ : a.name_)
  extern __shared__ __align__(16) float cf_smem[];
  float *img = cf_smem, *feat = cf_smem + CF_IMG_FLOATS;  // feat: [16][CF_FLD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kk = lane >> 4;
  int kind = 0, stride, np;
  int64_t field0, out_row;
  if (a.desc) {
    const rows_tile d = a.desc[blockIdx.x];
    kind = d.kind; stride = d.stride; np = d.count; field0 = d.start; out_row = d.out_row;
  } else {
    int tile = blockIdx.x;
    if (tile >= a.tiles[0]) { tile -= a.tiles[0]; kind = 1; }
    if (kind == 1 && tile >= a.tiles[1]) { tile -= a.tiles[1]; kind = 2; }
    stride = a.stride[kind];
    const int p0 = tile * 16;
    np = a.count[kind] - p0 < 16 ? a.count[kind] - p0 : 16;
    field0 = a.start[kind] + (int64_t)p0 * stride;
    out_row = p0;
  }
  const float *w4 = a.w4[kind];
  if constexpr (SET) ww_set_move(w4, set_off);  // (behind the choice by kind: the three pointers stay where the kernel arguments are)

  float4 wreg[CV_KB][2];
  float wlast[2], cb0, cb1;
  CV_LOAD_W(wreg, wlast, cb0, cb1, w4, RK_ARG(cbias))

  // ---- stage the union of the 16 fields: image[(mel + PF)][row - field0]
  int a_off[5], o_off[5][4];
  {
    constexpr int MAXV = 6;  // 6 * 256 float4 >= 140 * 40 / 4
    const int ncols = 15 * stride + CV_KT;
    const bool al16 = ((((uintptr_t)a.mel) & 15) == 0);
    float4 stage[MAXV];
    stage_loads(al16, [&](auto al) {
      constexpr bool AL = decltype(al)::value;
#pragma unroll
      for (int q = 0; q < MAXV; ++q) {
        const int f4 = q * CF_THREADS + tid, it = f4 / 10;
        const int64_t r = field0 + it, rc = r < 0 ? 0 : r < a.mel_rows ? r : a.mel_rows - 1;  // (the host checked: mel_rows >= T)
        stage[q] = ld_mel4_sel<AL>(a.mel + rc * CV_NMEL + (f4 - it * 10) * 4, it < ncols && r >= 0 && r < a.mel_rows);
      }
    });
    LDS_CLEAR16(img, CF_IMG_FLOATS / 4, CF_THREADS)
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int mt = wave + 4 * i, m = mt * 16 + j;   // 20 m-tiles: (position, frequency) rows
      const int p = m / CV_OF, f = m - p * CV_OF;
      a_off[i] = (f * CV_SF) * CV_LDT + p * stride;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int mo = mt * 16 + kk * 4 + r, po = mo / CV_OF, fo = mo - po * CV_OF;
        o_off[i][r] = po * CF_FLD + fo * 32 + j;
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MAXV; ++q) {
      const int f4 = q * CF_THREADS + tid, it = f4 / 10, im = (f4 - it * 10) * 4;
      if (it < ncols) {
        const float e[4] = {stage[q].x, stage[q].y, stage[q].z, stage[q].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) img[(im + c + CV_PF) * CV_LDT + it] = e[c];
      }
    }
  }
  __syncthreads();
  // ---- conv: five m-tiles per wave (CV_TILE_LOOP)
  {
    // An edge position's cleared taps (conv_wL: frames kt < PT, conv_wR: the last 7, model_pack.h) lie over rows of the buffer that
    // are NOT the window's - the sequence's own rows in front of it or behind it, a gap, the next sequence.  0 * x is 0 for a finite
    // x only, so the operands under those taps are cleared as well, by a select: a NaN or an Inf in a row the window does not name
    // stays out of it.  (Finite rows: the same +-0 products as before.)  `kind` is uniform: the interior tiles skip all of it.
    auto load_a = [&](cv_a &av, int i) {
      CV_LOAD_A(av, img + a_off[i])
      if (kind != 0) {
        const int lo = kind == 1 ? 0 : CV_KT - 7, hi = kind == 1 ? CV_PT : CV_KT;  // the cleared frames [lo, hi)
#pragma unroll
        for (int kb = 0; kb < CV_KB; ++kb) {
          const int kt = (kb * 16 + kk * 4) % CV_KT;
          av.q[kb].x = (kt + 0 >= lo && kt + 0 < hi) ? 0.f : av.q[kb].x;
          av.q[kb].y = (kt + 1 >= lo && kt + 1 < hi) ? 0.f : av.q[kb].y;
          av.q[kb].z = (kt + 2 >= lo && kt + 2 < hi) ? 0.f : av.q[kb].z;
          av.q[kb].w = (kt + 3 >= lo && kt + 3 < hi) ? 0.f : av.q[kb].w;
        }
        const int ktl = CV_QL * 4 % CV_KT + kk;  // the last quad's frames 16..19
        av.last = (ktl >= lo && ktl < hi) ? 0.f : av.last;
      }
    };
    auto store_tile = [&](int i, const f32x4 &r0, const f32x4 &r1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        feat[o_off[i][r]] = relu1(r0[r]);
        feat[o_off[i][r] + 16] = relu1(r1[r]);
      }
    };
    f32x4 prev0 = {0.f, 0.f, 0.f, 0.f}, prev1 = {0.f, 0.f, 0.f, 0.f};
    CV_TILE_LOOP(5, if (i > 0) store_tile(i - 1, prev0, prev1);)
    store_tile(4, prev0, prev1);
  }
  PJ_W_LANE(RK_ARG(wx1s))
  float4 bq[4][3];
  PJ_RING_PROLOGUE(4)
  __syncthreads();  // feat complete
  // ---- projection: 16 rows = one MFMA tile per n-tile, 3 n-tiles per wave
  {
    const float *a0p = feat + j * CF_FLD + kk * 4;
    f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float4 avq[2];
    avq[0] = *(const float4 *)(a0p);
    float bv1[3];
    PJ_LOAD_BIAS(bv1, RK_ARG(bx1))
    PJ_KLOOP(4, PJ_ROWS16, PJ_NO_ROWS, avq[(ks + 1) & 1] = *(const float4 *)(a0p + (ks + 1) * 16);)
    float *out = a.out[kind] + (size_t)out_row * 192;
    if constexpr (SET) out += (size_t)blockIdx.y * (size_t)set.aux[kind == 0 ? WW_SLIDE_AUX_NI : WW_SLIDE_AUX_NW] * 192;
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const int col = wave * 48 + n * 16 + j;
      const float bv = bv1[n];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (kk * 4 + r < np) out[(size_t)(kk * 4 + r) * 192 + col] = acc[n][r] + bv;
    }
  }
#undef RK_ARG
}

// ------------------------------------------------------------------------------------------
// crnn_fused_bf16_kernel (WW_PRECISION_BF16X3): phases A..C of crnn_fused_kernel on the bf16 matrix pipe with split
// operands, x = hi + lo (two bf16, 16 mantissa bits) and a*b = ah*bh + ah*bl + al*bh on v_mfma_f32_16x16x32_bf16 with
// fp32 accumulate - the arithmetic of the split-bf16 Wavenet (wavenet.hip).  48 matrix cycles per 16x16x32 products
// against 256 for eight v_mfma_f32_16x16x4_f32, and on a pipe that runs beside the vector ALU (the fp32 MFMA does not).
// Posteriors move by <= 1e-5 against the fp32 kernel (tests/test_gpu_parity.py); fp32 stays the default.
//   A  the window goes to LDS as two bf16 planes [mel + 1][frame + 8] (pairs of frames packed per 32-bit store)
//   B  conv TRANSPOSED: channels are the MFMA rows (weights = A operand), the 380 output positions its columns, so a
//      lane ends up with 4 consecutive channels of one position = one 8-byte store per plane into feat[t][f*32 + c].
//      K = (kf, kt'') with kt padded 20 -> 24 and shifted by 2, so that every group of 8 k is 16 aligned bytes of one
//      image row: 15 groups + 1 zero group = 4 k-steps of 32
//   C  projection: rows 0..15 and 16..18 (+13 clamped) as two MFMA row tiles, 3 n-tiles per wave, W_x1 hi/lo planes
//      streamed from L2 in B-operand order, two k-steps ahead
//   D..G as the fp32 kernel (cf_phases_d_to_g).
// ------------------------------------------------------------------------------------------
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
#define CB_LD 168   // image row, bf16 elements: frame + 8
#define CB_ROWS 43  // mel + 1
#define CB_FLD 648  // feat row, bf16 elements
#define CFB_IMG_FLOATS 7232  // two bf16 image planes (28,896 B) rounded up; the fp32 kernel's image region is 7,216 floats
#define CFB_SMEM_BYTES ((CFB_IMG_FLOATS + CF_FEAT_FLOATS) * 4)
static_assert(2 * CB_ROWS * CB_LD * 2 <= CFB_IMG_FLOATS * 4 && 2 * CV_OT * CB_FLD * 2 <= CF_FEAT_FLOATS * 4 && CF_W2S + 8 * 64 <= CFB_IMG_FLOATS,
              "bf16 planes / post-conv tenants exceed their LDS regions");

// (a, b) -> packed bf16 pairs hi and lo with a ~ hi.x + lo.x, b ~ hi.y + lo.y
__device__ __forceinline__ void split2_pair(float a, float b, unsigned &h, unsigned &l) {
  const bf16x2_t hh = __builtin_convertvector((f32x2_t){a, b}, bf16x2_t);
  h = __builtin_bit_cast(unsigned, hh);
  const bf16x2_t ll = __builtin_convertvector((f32x2_t){a - __uint_as_float(h << 16), b - __uint_as_float(h & 0xffff0000u)}, bf16x2_t);
  l = __builtin_bit_cast(unsigned, ll);
}

template <bool FRONT_ONLY>
__global__ __launch_bounds__(CF_THREADS, 2) void crnn_fused_bf16_kernel(fused_args a) {
  extern __shared__ __align__(16) float cf_smem[];
  float *img = cf_smem, *feat = cf_smem + CFB_IMG_FLOATS;
  unsigned short *imgh = (unsigned short *)img, *imgl = imgh + CB_ROWS * CB_LD;
  unsigned short *fth = (unsigned short *)feat, *ftl = fth + CV_OT * CB_FLD;
  constexpr int H = GR_H, OT = CV_OT, M = CV_OT * CV_OF;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kk = lane >> 4;
  const int w = blockIdx.x;
  int64_t row;
  int valid;
  window_span(a.wa, w, a.T, row, valid);

  // conv weights, A operand (rows = channels): [plane][k-step 4][m-tile 2][lane][8 bf16]
  uint4 wq[2][CWB_KS][CWB_MT];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int ks = 0; ks < CWB_KS; ++ks)
#pragma unroll
      for (int mt = 0; mt < CWB_MT; ++mt) wq[p][ks][mt] = ((const uint4 *)a.cwb)[((p * CWB_KS + ks) * CWB_MT + mt) * 64 + lane];
  float cb[2][4];  // bias of this lane's channels mt*16 + kk*4 + r
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) cb[mt][r] = a.cbias[mt * 16 + kk * 4 + r];

  // ---- A: stage the window as bf16 hi / lo planes; a thread owns (frame pair, mel quad) items
  int b_off[6], f_off[6];  // per position tile of this wave: image offset of (t, f), feat offset of (t, f); -1 past M
  {
    constexpr int NIT = 3;  // 3 * 256 >= 76 frame pairs * 10 mel quads
    const float *src = a.mel + row * CV_NMEL;
    const bool al16 = ((((uintptr_t)src) & 15) == 0);
    float4 lo4[NIT], hi4[NIT];
#pragma unroll
    for (int q = 0; q < NIT; ++q) lo4[q] = hi4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid > 0) stage_loads(al16, [&](auto al) {
      constexpr bool AL = decltype(al)::value;
#pragma unroll
      for (int q = 0; q < NIT; ++q) {
        const int item = q * CF_THREADS + tid, fp = item / 10, mq = item - fp * 10;
        const int f0 = 2 * fp, f1 = 2 * fp + 1;
        lo4[q] = ld_mel4_sel<AL>(src + (f0 < valid ? f0 : valid - 1) * CV_NMEL + mq * 4, f0 < valid);
        hi4[q] = ld_mel4_sel<AL>(src + (f1 < valid ? f1 : valid - 1) * CV_NMEL + mq * 4, f1 < valid);
      }
    });
    for (int i = tid; i < CFB_IMG_FLOATS / 4; i += CF_THREADS) ((float4 *)img)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int m = (wave + 4 * i) * 16 + j, mc = m < M ? m : M - 1;
      const int t = mc / CV_OF, f = mc - t * CV_OF;
      b_off[i] = (2 * f) * CB_LD + 8 * t;
      f_off[i] = m < M ? t * CB_FLD + f * 32 : -1;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NIT; ++q) {
      const int item = q * CF_THREADS + tid, fp = item / 10, mq = item - fp * 10;
      if (2 * fp < a.T) {
        const float x0[4] = {lo4[q].x, lo4[q].y, lo4[q].z, lo4[q].w}, x1[4] = {hi4[q].x, hi4[q].y, hi4[q].z, hi4[q].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          unsigned h, l;
          split2_pair(x0[c], x1[c], h, l);
          const int o = (mq * 4 + c + 1) * CB_LD + 2 * fp + 8;  // even: one aligned 32-bit store per plane
          *(unsigned *)(imgh + o) = h;
          *(unsigned *)(imgl + o) = l;
        }
      }
    }
  }
  __syncthreads();

  // ---- B: conv (transposed) -> feat planes
  {
    auto load_x = [&](bf16x8_t(&xh)[4], bf16x8_t(&xl)[4], int i) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        int G = ks * 4 + kk;
        G = G < 15 ? G : 14;  // the 16th group has zero weights: any valid address
        const int kf = G / 3, h8 = (G - kf * 3) * 8;
        const int o = b_off[i] + kf * CB_LD + h8;
        xh[ks] = *(const bf16x8_t *)(imgh + o);
        xl[ks] = *(const bf16x8_t *)(imgl + o);
      }
    };
    auto store_pos = [&](int i, const f32x4 (&r)[2]) {
      if (f_off[i] >= 0) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          unsigned h0, l0, h1, l1;
          split2_pair(fmaxf(r[mt][0], 0.f), fmaxf(r[mt][1], 0.f), h0, l0);
          split2_pair(fmaxf(r[mt][2], 0.f), fmaxf(r[mt][3], 0.f), h1, l1);
          const int o = f_off[i] + mt * 16 + kk * 4;
          *(uint2 *)(fth + o) = make_uint2(h0, h1);
          *(uint2 *)(ftl + o) = make_uint2(l0, l1);
        }
      }
    };
    bf16x8_t xh[2][4], xl[2][4];
    f32x4 prev[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    load_x(xh[0], xl[0], 0);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      if (i + 1 < 6) load_x(xh[(i + 1) & 1], xl[(i + 1) & 1], i + 1);
      f32x4 acc[2] = {{cb[0][0], cb[0][1], cb[0][2], cb[0][3]}, {cb[1][0], cb[1][1], cb[1][2], cb[1][3]}};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const bf16x8_t wh = __builtin_bit_cast(bf16x8_t, wq[0][ks][mt]), wl = __builtin_bit_cast(bf16x8_t, wq[1][ks][mt]);
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, xh[i & 1][ks], acc[mt], 0, 0, 0);
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xl[i & 1][ks], acc[mt], 0, 0, 0);
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xh[i & 1][ks], acc[mt], 0, 0, 0);
        }
      if (i > 0) store_pos(i - 1, prev);
      prev[0] = acc[0];
      prev[1] = acc[1];
    }
    store_pos(5, prev);
  }
  // W_x1 planes, B operand: [plane][k-step 20][n-tile 12][lane][8 bf16]; this wave's n-tiles are 3 wave .. 3 wave + 2
  auto w_ld = [&](int p, int ks, int n) { return ((const uint4 *)a.wx1b)[((size_t)(p * WX1B_KS + ks) * WX1B_NT + wave * 3 + n) * 64 + lane]; };
  uint4 bq[3][2][3];  // [ring slot][plane][n]
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int n = 0; n < 3; ++n) bq[s2][p][n] = w_ld(p, s2, n);
  __syncthreads();  // feat complete; the image is dead from here on
  float *gxs = img + CF_GX, *seq1 = img + CF_SEQ, *hb = img + CF_HB;
  for (int i = tid; i < 32 * GR_SEQ_LD; i += CF_THREADS) seq1[i] = 0.f;
  if (tid < 2 * 2 * 2 * H) hb[tid] = 0.f;

  // ---- C: layer-1 input projection
  const int unit = lane >> 1, half = lane & 1, dir = wave & 1;
  gru_w g;
  {
    const int r1 = 16 + j < OT ? 16 + j : OT - 1;  // rows 19..31 of the second row tile do not exist: clamped, never stored
    const unsigned short *a0h = fth + j * CB_FLD + kk * 8, *a0l = ftl + j * CB_FLD + kk * 8;
    const unsigned short *a1h = fth + r1 * CB_FLD + kk * 8, *a1l = ftl + r1 * CB_FLD + kk * 8;
    f32x4 acc[2][3];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int n = 0; n < 3; ++n) acc[mt][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float bv1[3];  // the biases of this lane's three columns: requested now, added when the products are complete
#pragma unroll
    for (int n = 0; n < 3; ++n) bv1[n] = a.bx1[wave * 48 + n * 16 + j];
    if (!FRONT_ONLY) gru_load_w(g, wave < 2 ? a.wh1 : a.wh2, wave < 2 ? a.bh1 : a.bh2, dir, unit, half);  // (in front of the projection)
#pragma unroll
    for (int ks = 0; ks < 20; ++ks) {
      if (ks + 2 < 20) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int n = 0; n < 3; ++n) bq[(ks + 2) % 3][p][n] = w_ld(p, ks + 2, n);
      }
      const bf16x8_t ah[2] = {*(const bf16x8_t *)(a0h + ks * 32), *(const bf16x8_t *)(a1h + ks * 32)};
      const bf16x8_t al[2] = {*(const bf16x8_t *)(a0l + ks * 32), *(const bf16x8_t *)(a1l + ks * 32)};
#pragma unroll
      for (int n = 0; n < 3; ++n) {
        const bf16x8_t bh = __builtin_bit_cast(bf16x8_t, bq[ks % 3][0][n]), bl = __builtin_bit_cast(bf16x8_t, bq[ks % 3][1][n]);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          acc[mt][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mt], bh, acc[mt][n], 0, 0, 0);
          acc[mt][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bl, acc[mt][n], 0, 0, 0);
          acc[mt][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bh, acc[mt][n], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const int col = wave * 48 + n * 16 + j;
      const float bv = bv1[n];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = mt * 16 + kk * 4 + r;
          if (t < OT) gxs[t * GR_GX_LD + col] = acc[mt][n][r] + bv;
        }
    }
  }
  __syncthreads();
  if (FRONT_ONLY) {
    float4 *dst = (float4 *)(a.gx_out + (size_t)w * OT * 6 * H);
    for (int q = tid; q < OT * 6 * H / 4; q += CF_THREADS) {
      const int e = q * 4, t = e / (6 * H), c = e - t * 6 * H;
      dst[q] = *(const float4 *)(&gxs[t * GR_GX_LD + c]);
    }
    return;
  }
  cf_phases_d_to_g(a, img, feat, g, w);
}

// ------------------------------------------------------------------------------------------
// gru_tail_kernel: everything behind the layer-1 input projections for one window in a TWO-wave workgroup (wave 0
// forward, wave 1 backward), for large batches: 22.7 KB of LDS, 128 registers and 2 waves per window put seven windows on a CU, so the
// strictly serial recurrences (38 steps of ~500 cycles) of fourteen waves interleave on the vector ALUs instead of one
// window's sitting beside another's fp32 MFMA stream (which runs on the same datapath: measured 2x slower steps).
// Phases as D..G of crnn_fused_kernel; the layer-2 projection takes its B operands straight from L2.
// ------------------------------------------------------------------------------------------
struct tail_args {
  const float *gx1;   // [Nw][OT][192], or nullptr: rows gathered from the three lists of crnn_rows_kernel
  const float *wh1, *bh1;
  const float *wx2s;  // B-operand order [16][192][4]
  const float *bx2, *wh2, *bh2, *w1, *b1, *w2, *b2;
  float *enc, *out;
  int NOUT, HEAD;
  const float *gxI, *gxL, *gxR;  // interior fields [..][192], left / right edge rows [Nw][192]
  int hop_g, eight_g;            // hop / g and 8 / g: position t of window w is interior field w * hop_g + (t - 1) * eight_g
  const int64_t *iI0;            // or: window w's first interior field explicitly (several sequences)
  const float *wx2;              // W_x2 row-major [2*3H][2H] (gru_tail16_kernel)
};
// LDS (floats): gx [19][196] | seq1 [20][68] (row 19 zero) | h [2][2][2][32] | enc [64] | hid [64] = 21.9 KB: seven per CU whatever
// the allocation granularity (22.7 KB with a 20th gx row was seven only if LDS is handed out in units below 1 KB)
#define GT_SEQ (19 * GR_GX_LD)
#define GT_HB (GT_SEQ + 20 * GR_SEQ_LD)
#define GT_ENC (GT_HB + 2 * 2 * 2 * GR_H)
#define GT_HID (GT_ENC + 2 * GR_H)
#define GT_SMEM_FLOATS (GT_HID + 2 * GR_H)

// SET (both tails; the grid's y is the call's member slot as in crnn_rows_kernel<SET>): the weights of member set.ids[blockIdx.y],
// plane blockIdx.y of the three projected-row lists and of the output; blockIdx.x stays the window (tail16: the group of sixteen -
// a group never mixes members), and iI0, a function of the geometry and the hop, serves every slot.
__device__ __forceinline__ void gt_set_move(tail_args &a, const ww_set_ref &set, int slot) {
  const long long off = ww_set_offset(set, slot);
  ww_set_move(a.wh1, off); ww_set_move(a.bh1, off); ww_set_move(a.wx2s, off); ww_set_move(a.wx2, off); ww_set_move(a.bx2, off);
  ww_set_move(a.wh2, off); ww_set_move(a.bh2, off); ww_set_move(a.w1, off); ww_set_move(a.b1, off); ww_set_move(a.w2, off);
  ww_set_move(a.b2, off);
  const size_t nI = (size_t)set.aux[WW_SLIDE_AUX_NI], nW = (size_t)set.aux[WW_SLIDE_AUX_NW], W = (size_t)set.aux[WW_SLIDE_AUX_W];
  a.gxI += (size_t)slot * nI * 6 * GR_H;
  a.gxL += (size_t)slot * nW * 6 * GR_H;
  a.gxR += (size_t)slot * nW * 6 * GR_H;
  a.out += (size_t)slot * W * a.NOUT;
}

template <bool SET = false>
__global__ __launch_bounds__(128, 4) void gru_tail_kernel(tail_args a, ww_set_ref set) {
  if constexpr (SET) gt_set_move(a, set, blockIdx.y);
  constexpr int H = GR_H, OT = CV_OT;
  __shared__ __align__(16) float sm[GT_SMEM_FLOATS];
  float *gxs = sm, *seq1 = sm + GT_SEQ, *hb = sm + GT_HB, *encs = sm + GT_ENC, *hid = sm + GT_HID;
  const int tid = threadIdx.x, lane = tid & 63, dir = wave_index(tid);  // (scalar)
  const int j = lane & 15, kk = lane >> 4, unit = lane >> 1, half = lane & 1;
  const int w = blockIdx.x;
  gru_w g;
  gru_load_w(g, a.wh1, a.bh1, dir, unit, half);
  {
    // the window's 19 projected rows -> LDS: all of a thread's 16-byte loads first (unconditional, the last ones clamped), then
    // the stores - as a loop of "load, store" every element was a round trip to L2 of its own, eight in a row per window
    constexpr int NQ = OT * 6 * H / 4, NS = (NQ + 127) / 128;
    int64_t i0w = (int64_t)w * a.hop_g;
    if (!a.gx1 && a.iI0) i0w = a.iI0[w];
    f32x4 st[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int q = min(tid + 128 * s, NQ - 1), t = q / 48, c4 = q - t * 48;
      const float *row = a.gx1 ? a.gx1 + ((size_t)w * OT + t) * 6 * H
                       : t == 0 ? a.gxL + (size_t)w * 6 * H
                       : t == OT - 1 ? a.gxR + (size_t)w * 6 * H
                                     : a.gxI + ((size_t)i0w + (size_t)(t - 1) * a.eight_g) * 6 * H;
      st[s] = *(const f32x4 *)(row + c4 * 4);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int q = tid + 128 * s, t = q / 48, c4 = q - t * 48;
      if (q < NQ) *(f32x4 *)(&gxs[t * GR_GX_LD + c4 * 4]) = st[s];
    }
  }
  CLEAR_SEQ_H(seq1, 20, hb, 128)
  __syncthreads();
  cf_recurrence<true>(g, gxs, hb + dir * 2 * H, seq1, dir, unit, half);
  __syncthreads();
  // layer-2 input projection: wave d owns n-tiles 6 d .. 6 d + 5, in two passes of three
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    const int nt0 = dir * 6 + pass * 3;
    float4 bq[4][3];
    L2_LOAD_W(bq, a.wx2s, nt0)
    float bb2[3];  // the biases with the weights
    L2_LOAD_BIAS(bb2, a.bx2, nt0)
    // between products and stores, pass 0: both waves are done reading gx1 before anybody overwrites it (gx2 takes its place)
    L2_PROJECT(bq, bb2, j < 3 ? 16 + j : 19 /* row 19 is zero */, nt0, __syncthreads();)
  }
  // layer-2 recurrent weights: requested only now, when the projection's operands are dead - the kernel fits 128 registers
  // (four waves per SIMD instead of three); one L2 latency per window, partly behind the barrier
  gru_w g2;
  gru_load_w(g2, a.wh2, a.bh2, dir, unit, half);
  __syncthreads();
  const float h_last = cf_recurrence<false>(g2, gxs, hb + (2 + dir) * 2 * H, nullptr, dir, unit, half);
  if (half == 0) {
    encs[dir * H + unit] = h_last;
    if (a.enc) a.enc[(size_t)w * 2 * H + dir * H + unit] = h_last;
  }
  __syncthreads();
  if (dir == 0) {  // detect head, w1 row `lane` straight from L2 (16 KB, shared by every workgroup)
    const float b1v = a.b1[lane], b2v = a.b2[lane < a.NOUT ? lane : 0];
    float acc = 0.f;  // one chain in k order: bit-identical to crnn_fused_kernel's head
    const float4 *wr = (const float4 *)(a.w1 + (size_t)lane * 2 * H);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float4 wv = wr[q];
      const float4 ev = *(const float4 *)(&encs[q * 4]);
      acc = fmaf(wv.x, ev.x, acc); acc = fmaf(wv.y, ev.y, acc);
      acc = fmaf(wv.z, ev.z, acc); acc = fmaf(wv.w, ev.w, acc);
    }
    hid[lane] = fmaxf(acc + b1v, 0.f);
    wsync_g();
    float y = 0.f;
    if (lane < a.NOUT) {
      for (int k = 0; k < 2 * H; ++k) y = fmaf(a.w2[lane * 64 + k], hid[k], y);
      y += b2v;
    }
    const float p = head_activation(y, lane, a.NOUT, a.HEAD);
    if (lane < a.NOUT) a.out[(size_t)w * a.NOUT + lane] = p;
  }
}

// ------------------------------------------------------------------------------------------
// gru_tail_ctc_kernel: gru_tail_kernel for a CTC-trained CRNN (Arik_CRNN_CTC, wwdetect/CRNN/model.py:82-145; WW_HEAD_CTC).  The same
// two-wave workgroup per window, the same sourcing of the 19 projected rows (its launcher hands it gx1: ww_k_crnn_ctc_forward), layer 1 and layer 2's input projection through the same
// macros - every step of layer 2 carries the bits the other tails give it.  What differs is behind them:
//   layer 2 keeps its step outputs (cf_recurrence<true>) in a second sequence buffer seq2[19][GR_SEQ_LD]: row t = [h_fwd(t) | h_bwd(t)],
//     the backward state at t being the one after steps 18..t (Keras' Bidirectional(return_sequences=True)); optional store enc [n][19][64]
//   the head is ONE dense layer on every row, z[t][c] = b2[c] + sum_k w2[c][k] seq2[t][k], then the softmax over the L classes of a
//     row; the 19 x 8 (row, class slot) pairs are dealt over the 128 threads in two passes, eight adjacent lanes per row, which is
//     the arrangement head_activation's softmax exchanges in; optional store steps [n][19][L]
//   thread 0 decodes the 19 rows of posteriors as written (ctc_decode.h): labels [n][max_labels], lengths [n]
// LDS (floats): gx [19][196] | seq1 [20][68] | seq2 [19][68] | h [2][2][2][32] | posteriors [19][8] = 27.1 KB: five workgroups per CU
// (the head's weights [8][68] take gx's place once layer 2 is done).
// ------------------------------------------------------------------------------------------
struct tail_ctc_args {
  tail_args t;        // t.enc: optional [Nw][OT][2H]; t.out is not used; t.NOUT = L (2..8), the blank is class L - 1
  float *steps;       // optional [Nw][OT][L]
  int32_t *labels;    // [Nw][max_labels]
  int32_t *lengths;   // [Nw]
  int max_labels;     // 1..OT
};
#define GTC_SEQ2 (GT_SEQ + 20 * GR_SEQ_LD)
#define GTC_HB (GTC_SEQ2 + 19 * GR_SEQ_LD)
#define GTC_POST (GTC_HB + 2 * 2 * 2 * GR_H)
#define GTC_SMEM_FLOATS (GTC_POST + 19 * 8)
static_assert(CV_OT == 19 && GTC_SEQ2 % 4 == 0 && GTC_HB % 4 == 0, "gru_tail_ctc_kernel's LDS layout is written for 19 steps, 16-byte aligned rows");

__global__ __launch_bounds__(128, 4) void gru_tail_ctc_kernel(tail_ctc_args ca) {
  const tail_args &a = ca.t;
  constexpr int H = GR_H, OT = CV_OT;
  __shared__ __align__(16) float sm[GTC_SMEM_FLOATS];
  float *gxs = sm, *seq1 = sm + GT_SEQ, *seq2 = sm + GTC_SEQ2, *hb = sm + GTC_HB, *post = sm + GTC_POST;
  const int tid = threadIdx.x, lane = tid & 63, dir = wave_index(tid);  // (scalar)
  const int j = lane & 15, kk = lane >> 4, unit = lane >> 1, half = lane & 1;
  const int w = blockIdx.x;
  gru_w g;
  gru_load_w(g, a.wh1, a.bh1, dir, unit, half);
  {
    // the window's 19 projected rows -> LDS, as gru_tail_kernel stages them
    constexpr int NQ = OT * 6 * H / 4, NS = (NQ + 127) / 128;
    int64_t i0w = (int64_t)w * a.hop_g;
    if (!a.gx1 && a.iI0) i0w = a.iI0[w];
    f32x4 st[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int q = min(tid + 128 * s, NQ - 1), t = q / 48, c4 = q - t * 48;
      const float *row = a.gx1 ? a.gx1 + ((size_t)w * OT + t) * 6 * H
                       : t == 0 ? a.gxL + (size_t)w * 6 * H
                       : t == OT - 1 ? a.gxR + (size_t)w * 6 * H
                                     : a.gxI + ((size_t)i0w + (size_t)(t - 1) * a.eight_g) * 6 * H;
      st[s] = *(const f32x4 *)(row + c4 * 4);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int q = tid + 128 * s, t = q / 48, c4 = q - t * 48;
      if (q < NQ) *(f32x4 *)(&gxs[t * GR_GX_LD + c4 * 4]) = st[s];
    }
  }
  CLEAR_SEQ_H(seq1, 20, hb, 128)
  __syncthreads();
  cf_recurrence<true>(g, gxs, hb + dir * 2 * H, seq1, dir, unit, half);
  __syncthreads();
  // layer-2 input projection: wave d owns n-tiles 6 d .. 6 d + 5, in two passes of three (gru_tail_kernel's)
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    const int nt0 = dir * 6 + pass * 3;
    float4 bq[4][3];
    L2_LOAD_W(bq, a.wx2s, nt0)
    float bb2[3];
    L2_LOAD_BIAS(bb2, a.bx2, nt0)
    L2_PROJECT(bq, bb2, j < 3 ? 16 + j : 19 /* row 19 is zero */, nt0, __syncthreads();)
  }
  gru_w g2;
  gru_load_w(g2, a.wh2, a.bh2, dir, unit, half);
  __syncthreads();
  // the head's weights: on their way during the recurrence (ctc_head_w_load)
  const float4 w2q = ctc_head_w_load(a.w2, tid, a.NOUT);
  // layer 2, every step kept: each (row, direction half) of seq2 is written exactly once, so seq2 needs no clearing
  cf_recurrence<true>(g2, gxs, hb + (2 + dir) * 2 * H, seq2, dir, unit, half);
  __syncthreads();
  // gx is dead: the head's weights take its place
  float *w2s = gxs;
  ctc_head_w_park(w2s, tid, w2q);
  if (a.enc)
    for (int i = tid; i < OT * 2 * H; i += 128) a.enc[(size_t)w * OT * 2 * H + i] = seq2[(i >> 6) * GR_SEQ_LD + (i & 63)];
  __syncthreads();
  // the shared head (ctc_head_slot): slot p = tid + 128 pass, two passes
  {
    const int L = a.NOUT, o = tid & 7;
    const float b2v = a.b2[o < L ? o : 0];
    float *steps_w = ca.steps ? ca.steps + (size_t)w * OT * L : nullptr;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) ctc_head_slot(w2s, seq2, b2v, tid + 128 * pass, L, post, steps_w);
  }
  __syncthreads();
  // greedy decode of the posteriors as written
  if (tid == 0)
    ca.lengths[w] = ww_ctc_greedy_row(post, OT, a.NOUT, 8, ca.labels + (size_t)w * ca.max_labels, ca.max_labels);
}

// the decode alone over [n][T][L] posteriors in global memory: one thread per sequence
__global__ __launch_bounds__(64) void ctc_greedy_kernel(const float *steps, long long n, int T, int L, int max_labels, int32_t *labels,
                                                        int32_t *lengths) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i < n) lengths[i] = ww_ctc_greedy_row(steps + (size_t)i * T * L, T, L, L, labels + (size_t)i * max_labels, max_labels);
}

// ------------------------------------------------------------------------------------------
// gru_tail16_kernel: the same work as gru_tail_kernel for SIXTEEN windows per two-wave workgroup (wave 0 forward, wave 1
// backward), with the recurrent mat-vec of the sixteen windows as one matrix product per step on v_mfma_f32_16x16x4_f32:
//   [16 windows x 32 units] x W_h^T [32 x 96]  =  6 n-tiles (z, r, c  x  unit half) x 8 k-steps = 48 MFMAs.
// A tile's accumulator has its unit (column) on the lane and four windows (rows) in its registers, and so do the tiles
// of the other gates - the gate arithmetic of a (window, unit) pair is lane-local, evaluated ONCE (gru_tail_kernel's lane
// pairs each evaluate a unit's gates twice), the projected inputs gx[window][t][gate unit] are read straight from global
// memory / L2 in that layout (one step ahead), and a step's new state goes through 2 KB of LDS to become the next step's A
// operand (lane = window, its eight k's of every k-step = eight consecutive units: two 16-byte reads).
// Layer 2's input projection (as many MFMAs as all four recurrences together) is computed per step in the same
// accumulators: A = seq1[t] of the sixteen windows (global workspace, written by layer 1), B = this direction's 96 rows of
// W_x2 held in registers (6 tiles x 16 k-steps), issued for step t+1 between writing h(t) and reading it back.
// Every sum is associated exactly as the vector form associates it (gru_step's four chains per gate; phase E's one chain per
// projected value, bias last) - v_mfma_f32_16x16x4_f32 is an fmaf chain in k order - so a window's posterior is the same bits
// whichever tail it was given to (tests/test_gpu_parity.py::test_crnn_large_batch_path).
// ------------------------------------------------------------------------------------------
#define GT16_LD 36   // h exchange row: 32 units + 4
#define GT16_ELD 68  // enc / hid row: 64 + 4
#define GT16_SMEM_BYTES ((2 * 2 * 16 * GT16_LD + 2 * 6 * 2 * 64 * 4) * 4)
struct tail16_args {
  tail_args t;
  float *seq;  // [workgroup][OT][16][64] layer-1 outputs
  int nw;      // windows in this launch (the last workgroup may be partial)
};

template <bool SET = false>
__global__ __launch_bounds__(128, 2) void gru_tail16_kernel(tail16_args aa, ww_set_ref set) {
  if constexpr (SET) {
    gt_set_move(aa.t, set, blockIdx.y);
    aa.seq += (size_t)blockIdx.y * (size_t)((aa.nw + 15) / 16) * CV_OT * 16 * 2 * GR_H;  // the slot's plane of the layer-1 outputs
  }
  constexpr int H = GR_H, OT = CV_OT;
  const tail_args &a = aa.t;
  // LDS: the h exchange (9.2 KB) + each wave's recurrent weights as B-operand pages [tile 6][half 2][lane 64] x 16 bytes
  // (24.6 KB: every lane reads back only what it wrote - 48 registers' worth that the four chains per tile need elsewhere);
  // the head's enc / hid rows move into the dead pages at the end.  33.8 KB: four workgroups per CU, as the registers allow
  extern __shared__ __align__(16) float sm16[];
  float (*hs)[2][16 * GT16_LD] = (float (*)[2][16 * GT16_LD])sm16;
  float *encs = sm16 + 2 * 2 * 16 * GT16_LD, *hid = encs + 16 * GT16_ELD;
  static_assert(2 * 16 * GT16_ELD <= 2 * 6 * 2 * 64 * 4, "enc / hid rows do not fit the weight pages");
  const int tid = threadIdx.x, lane = tid & 63, dir = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  float4 *whl = (float4 *)(sm16 + 2 * 2 * 16 * GT16_LD) + (size_t)dir * 6 * 2 * 64 + lane;  // this lane's slot of page 0
  const int w0 = blockIdx.x * 16;
  float *seq = aa.seq + (size_t)blockIdx.x * OT * 16 * 2 * H;

  // rows of the accumulator tiles = windows 4 g + r (clamped in a partial workgroup: computed twice, stored once)
  int wi[4];
  int64_t i0[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) wi[r] = min(w0 + 4 * g + r, aa.nw - 1);
  if (!a.gx1 && a.iI0) {  // (one uniform branch around four loads in flight; as a per-row ternary they were four round trips in a row)
#pragma unroll
    for (int r = 0; r < 4; ++r) i0[r] = a.iI0[wi[r]];
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) i0[r] = a.gx1 ? 0 : (int64_t)wi[r] * a.hop_g;
  }
  auto gx_row = [&](int r, int t) -> const float * {
    if (a.gx1) return a.gx1 + ((size_t)wi[r] * OT + t) * 6 * H;
    if (t == 0) return a.gxL + (size_t)wi[r] * 6 * H;
    if (t == OT - 1) return a.gxR + (size_t)wi[r] * 6 * H;
    return a.gxI + (size_t)(i0[r] + (int64_t)(t - 1) * a.eight_g) * 6 * H;
  };
  // recurrent weights as B operands: tile nt = gate * 2 + unit half.  The eight MFMAs of a tile and step are the four chains
  // of gru_step, two MFMAs each: chain (hh, p) = units 16 hh + p, + 2, .. + 14; its MFMA q takes the k-lanes g = 0..3 <-> unit
  // u = 16 hh + 8 q + 2 g + p.  Operand slot i = 4 hh + 2 q + p; in the LDS exchange row unit u sits at GT16_POS(u) =
  // 8 g + i, so that a lane group reads its eight operands as two 16-byte words.
#define GT16_POS(u_) (8 * (((u_) >> 1) & 3) + 4 * ((u_) >> 4) + 2 * (((u_) >> 3) & 1) + ((u_) & 1))
  float bh[6];
  auto load_wh = [&](const float *whp, const float *bhp) {
#pragma unroll
    for (int nt = 0; nt < 6; ++nt) {
      const int row = (nt >> 1) * H + (nt & 1) * 16 + c;
      const float *p = whp + ((size_t)dir * 3 * H + row) * H + 2 * g;
      float wv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) wv[i] = p[16 * (i >> 2) + 8 * ((i >> 1) & 1) + (i & 1)];
      whl[(2 * nt) * 64] = make_float4(wv[0], wv[1], wv[2], wv[3]);
      whl[(2 * nt + 1) * 64] = make_float4(wv[4], wv[5], wv[6], wv[7]);
      bh[nt] = bhp[dir * 3 * H + row];
    }
  };
  // pre[nt] = pre-activation of tile nt for the four windows of this lane: (E0 + O0) + (E1 + O1), E0 starting from X0_[nt] (the
  // projected input of the z and r gates; zeros for c), O0 from b_h, the others from zero.  A tile's operands are read from
  // its page while the previous tile's MFMAs run; one tile's chains at a time (all six at once would need 96 registers)
#define GT16_PRE_ALL(X0_)                                                                          \
  {                                                                                                \
    float4 wb[2][2];                                                                               \
    wb[0][0] = whl[0];                                                                             \
    wb[0][1] = whl[64];                                                                            \
    _Pragma("unroll") for (int nt = 0; nt < 6; ++nt) {                                             \
      if (nt + 1 < 6) {                                                                            \
        wb[(nt + 1) & 1][0] = whl[(2 * nt + 2) * 64];                                              \
        wb[(nt + 1) & 1][1] = whl[(2 * nt + 3) * 64];                                              \
      }                                                                                            \
      __builtin_amdgcn_sched_barrier(0);                                                           \
      const float4 b0 = wb[nt & 1][0], b1 = wb[nt & 1][1];                                         \
      f32x4 e0 = nt < 4 ? X0_[nt < 4 ? nt : 0] : zero4, o0 = {bh[nt], bh[nt], bh[nt], bh[nt]};     \
      e0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[0], b0.x, e0, 0, 0, 0);                         \
      o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[1], b0.y, o0, 0, 0, 0);                         \
      e0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[2], b0.z, e0, 0, 0, 0);                         \
      o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[3], b0.w, o0, 0, 0, 0);                         \
      f32x4 e1 = zero4, o1 = zero4;                                                                \
      e1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[4], b1.x, e1, 0, 0, 0);                         \
      o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[5], b1.y, o1, 0, 0, 0);                         \
      e1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[6], b1.z, e1, 0, 0, 0);                         \
      o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[7], b1.w, o1, 0, 0, 0);                         \
      pre[nt] = (e0 + o0) + (e1 + o1);                                                             \
      __builtin_amdgcn_sched_barrier(0);                                                           \
    }                                                                                              \
  }
  // the first step: h = 0, the chains are their initial values (0 * w adds nothing, so the products are skipped)
#define GT16_PRE_FIRST(X0_)                                                                        \
  _Pragma("unroll") for (int nt = 0; nt < 6; ++nt) {                                               \
    const f32x4 o0 = {bh[nt], bh[nt], bh[nt], bh[nt]};                                             \
    pre[nt] = ((nt < 4 ? X0_[nt < 4 ? nt : 0] : zero4) + o0) + (zero4 + zero4);                    \
  }
  load_wh(a.wh1, a.bh1);
  for (int i = tid; i < 2 * 2 * 16 * GT16_LD; i += 128) (&hs[0][0][0])[i] = 0.f;
  const int pos0 = GT16_POS(c), pos1 = GT16_POS(16 + c);  // where this lane's two units sit in an exchange row

  // ---- layer 1 ------------------------------------------------------------------------------
  float h_own[4][2];  // [row r][unit half]: h of (window 4 g + r, unit 16 uh + c)
#pragma unroll
  for (int r = 0; r < 4; ++r) h_own[r][0] = h_own[r][1] = 0.f;
  float gxn[4][6];
  {
    const int t = dir ? OT - 1 : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float *row = gx_row(r, t) + dir * 3 * H + c;
#pragma unroll
      for (int nt = 0; nt < 6; ++nt) gxn[r][nt] = row[(nt >> 1) * H + (nt & 1) * 16];
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int s = 0; s < OT; ++s) {
    const int t = dir ? OT - 1 - s : s, cur = s & 1;
    f32x4 x0[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) x0[nt] = (f32x4){gxn[0][nt], gxn[1][nt], gxn[2][nt], gxn[3][nt]};
    float gxc[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r) { gxc[r][0] = gxn[r][4]; gxc[r][1] = gxn[r][5]; }
    if (s + 1 < OT) {  // next step's projected inputs: in flight during this step's products and gates
      const int tn = dir ? t - 1 : t + 1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float *row = gx_row(r, tn) + dir * 3 * H + c;
#pragma unroll
        for (int nt = 0; nt < 6; ++nt) gxn[r][nt] = row[(nt >> 1) * H + (nt & 1) * 16];
      }
    }
    f32x4 pre[6];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
      const float4 *hp = (const float4 *)(&hs[dir][cur][c * GT16_LD + 8 * g]);
      const float4 a0 = hp[0], a1 = hp[1];
      const float ha[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      GT16_PRE_ALL(x0)
    } else {
      GT16_PRE_FIRST(x0)
    }
#pragma unroll
    for (int uh = 0; uh < 2; ++uh)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = fast_sigmoid(pre[uh][r]);
        const float rr = fast_sigmoid(pre[2 + uh][r]);
        const float hn = gru_blend(z, h_own[r][uh], gru_candidate(rr, pre[4 + uh][r], gxc[r][uh]));
        h_own[r][uh] = hn;
        hs[dir][cur ^ 1][(4 * g + r) * GT16_LD + (uh ? pos1 : pos0)] = hn;
        seq[((size_t)t * 16 + 4 * g + r) * 2 * H + dir * H + uh * 16 + c] = hn;
      }
    wsync_h();
  }
  __syncthreads();  // seq1 of both directions is in memory (workgroup scope)

  // ---- layer 2: the input projection of step t+1 is issued between writing h(t) and reading it back ---------------------
  // gx2[t][window][n] as phase E of crnn_fused_kernel computes it: ONE fmaf chain from zero over k = 16 kb + 4 kk + e in the
  // order kb, e, kk (kk = the k-lane), the bias added last.  A = seq1[t] of the sixteen windows (global workspace, written by
  // layer 1), B = this direction's 96 rows of W_x2 in registers: slot 4 kb + e of lane group g <-> column 16 kb + 4 g + e
  load_wh(a.wh2, a.bh2);
  float wx[6][16];
  float bx[6];
#pragma unroll
  for (int nt = 0; nt < 6; ++nt) {
    const int row = dir * 3 * H + (nt >> 1) * H + (nt & 1) * 16 + c;
    const float4 *p = (const float4 *)(a.wx2 + (size_t)row * 2 * H + 4 * g);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = p[4 * q];
      wx[nt][4 * q] = v.x; wx[nt][4 * q + 1] = v.y; wx[nt][4 * q + 2] = v.z; wx[nt][4 * q + 3] = v.w;
    }
    bx[nt] = a.bx2[row];
  }
  for (int i = tid; i < 2 * 2 * 16 * GT16_LD; i += 128) (&hs[0][0][0])[i] = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) h_own[r][0] = h_own[r][1] = 0.f;
  f32x4 gx2[6];  // projected inputs of the step at hand: tiles 0..3 start the z and r chains, 4..5 are the candidate's x part
  auto project = [&](int t) {
    const float4 *sp = (const float4 *)(seq + ((size_t)t * 16 + c) * 2 * H + 4 * g);
    const float4 q0 = sp[0], q1 = sp[4], q2 = sp[8], q3 = sp[12];
#pragma unroll
    for (int nt = 0; nt < 6; ++nt) gx2[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#define GT16_PROJ(q_, kb_)                                                                           \
  _Pragma("unroll") for (int nt = 0; nt < 6; ++nt) gx2[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(q_.x, wx[nt][4 * kb_ + 0], gx2[nt], 0, 0, 0); \
  _Pragma("unroll") for (int nt = 0; nt < 6; ++nt) gx2[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(q_.y, wx[nt][4 * kb_ + 1], gx2[nt], 0, 0, 0); \
  _Pragma("unroll") for (int nt = 0; nt < 6; ++nt) gx2[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(q_.z, wx[nt][4 * kb_ + 2], gx2[nt], 0, 0, 0); \
  _Pragma("unroll") for (int nt = 0; nt < 6; ++nt) gx2[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(q_.w, wx[nt][4 * kb_ + 3], gx2[nt], 0, 0, 0);
    GT16_PROJ(q0, 0)
    GT16_PROJ(q1, 1)
    GT16_PROJ(q2, 2)
    GT16_PROJ(q3, 3)
#undef GT16_PROJ
#pragma unroll
    for (int nt = 0; nt < 6; ++nt) gx2[nt] += (f32x4){bx[nt], bx[nt], bx[nt], bx[nt]};
  };
  project(dir ? OT - 1 : 0);
  __syncthreads();
#pragma unroll 1
  for (int s = 0; s < OT; ++s) {
    const int t = dir ? OT - 1 - s : s, cur = s & 1;
    f32x4 pre[6];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
      const float4 *hp = (const float4 *)(&hs[dir][cur][c * GT16_LD + 8 * g]);
      const float4 a0 = hp[0], a1 = hp[1];
      const float ha[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      GT16_PRE_ALL(gx2)
    } else {
      GT16_PRE_FIRST(gx2)
    }
#pragma unroll
    for (int uh = 0; uh < 2; ++uh)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = fast_sigmoid(pre[uh][r]);
        const float rr = fast_sigmoid(pre[2 + uh][r]);
        const float hn = gru_blend(z, h_own[r][uh], gru_candidate(rr, pre[4 + uh][r], gx2[4 + uh][r]));
        h_own[r][uh] = hn;
        hs[dir][cur ^ 1][(4 * g + r) * GT16_LD + (uh ? pos1 : pos0)] = hn;
      }
    if (s + 1 < OT) project(dir ? t - 1 : t + 1);  // between the h write and its read-back: covers the LDS round trip
    wsync_h();
  }
  __syncthreads();  // both waves are done with their weight pages: enc / hid take their place
#pragma unroll
  for (int uh = 0; uh < 2; ++uh)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      encs[(4 * g + r) * GT16_ELD + dir * H + uh * 16 + c] = h_own[r][uh];
      if (a.enc && w0 + 4 * g + r < aa.nw) a.enc[(size_t)(w0 + 4 * g + r) * 2 * H + dir * H + uh * 16 + c] = h_own[r][uh];
    }
  __syncthreads();

  // ---- detect head: wave d takes windows 8 d .. 8 d + 7; lane = hidden unit, its w1 row in registers -----
  {
    float4 w1r[16];
    const float4 *wr = (const float4 *)(a.w1 + (size_t)lane * 2 * H);
#pragma unroll
    for (int q = 0; q < 16; ++q) w1r[q] = wr[q];
    const float b1v = a.b1[lane];
#pragma unroll 1
    for (int wq = dir * 8; wq < dir * 8 + 8; ++wq) {
      float acc = 0.f;  // one chain in k order: bit-identical to crnn_fused_kernel's head
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float4 ev = *(const float4 *)(&encs[wq * GT16_ELD + q * 4]);
        acc = fmaf(w1r[q].x, ev.x, acc); acc = fmaf(w1r[q].y, ev.y, acc);
        acc = fmaf(w1r[q].z, ev.z, acc); acc = fmaf(w1r[q].w, ev.w, acc);
      }
      hid[wq * GT16_ELD + lane] = fmaxf(acc + b1v, 0.f);
    }
  }
  __syncthreads();
  {
    const int wq = tid >> 3, o = tid & 7;  // 16 windows x up to 8 outputs
    float y = 0.f;
    if (o < a.NOUT) {
      for (int k = 0; k < 2 * H; ++k) y = fmaf(a.w2[o * 64 + k], hid[wq * GT16_ELD + k], y);
      y += a.b2[o];
    }
    const float p = head_activation(y, o, a.NOUT, a.HEAD);
    if (o < a.NOUT && w0 + wq < aa.nw) a.out[(size_t)(w0 + wq) * a.NOUT + o] = p;
  }
}


#undef CF_ROUND_L2
#undef L2_PROJECT
#undef PJ_KLOOP
#undef PJ_ROWS16
#undef PJ_ROWS3
#undef PJ_NO_ROWS
#undef CV_TILE_LOOP
#undef CV_MFMA_KB
#undef CV_MFMA_LAST
#undef GT16_PRE_ALL
#undef GT16_PRE_FIRST
#undef GT16_POS

// detect.tflite alone (reference detect_model(x), wakeword/tflite.py:228-229): one wave per row
__global__ __launch_bounds__(64) void crnn_detect_kernel(const float *enc, const float *w1, const float *b1, const float *w2,
                                                         const float *b2, float *out, int NOUT, int HEAD) {
  __shared__ float e[64], hid[64];
  const int lane = threadIdx.x, w = blockIdx.x;
  e[lane] = enc[(size_t)w * 64 + lane];
  __syncthreads();
  float acc = 0.f;
  for (int k = 0; k < 64; ++k) acc = fmaf(w1[lane * 64 + k], e[k], acc);
  hid[lane] = fmaxf(acc + b1[lane], 0.f);
  __syncthreads();
  float y = 0.f;
  if (lane < NOUT) {
    for (int k = 0; k < 64; ++k) y = fmaf(w2[lane * 64 + k], hid[k], y);
    y += b2[lane];
  }
  const float p = head_activation(y, lane, NOUT, HEAD);
  if (lane < NOUT) out[(size_t)w * NOUT + lane] = p;
}

// The detect head at any width: enc [Nw][E] (E = 2H <= 128) -> Dense(F <= 64, relu) -> Dense(NOUT <= 8) -> sigmoid | softmax, one wave
// per row.  crnn_detect_kernel's association: one fmaf chain in k order from zero, the bias last, then head_activation.
__global__ __launch_bounds__(64) void crnn_head_kernel(const float *enc, const float *w1, const float *b1, const float *w2, const float *b2,
                                                       float *out, int E, int F, int NOUT, int HEAD) {
  __shared__ float e[128], hid[64];
  const int lane = threadIdx.x, w = blockIdx.x;
  for (int k = lane; k < E; k += 64) e[k] = enc[(size_t)w * E + k];
  __syncthreads();
  if (lane < F) {
    float acc = 0.f;
    for (int k = 0; k < E; ++k) acc = fmaf(w1[lane * E + k], e[k], acc);
    hid[lane] = fmaxf(acc + b1[lane], 0.f);
  }
  __syncthreads();
  float y = 0.f;
  if (lane < NOUT) {
    for (int k = 0; k < F; ++k) y = fmaf(w2[lane * F + k], hid[k], y);
    y += b2[lane];
  }
  const float p = head_activation(y, lane, NOUT, HEAD);
  if (lane < NOUT) out[(size_t)w * NOUT + lane] = p;
}

// the cell every kernel above rnn_layer_kernel is written for
static bool crnn_std_cell(const ww_crnn_dev &c) { return c.CELL == WW_CELL_GRU && c.H == GR_H && c.F == 2 * GR_H; }

// A CTC-trained CRNN (WW_HEAD_CTC) has no Dense(64, relu) -> Dense(n_out) head on its last states: every launcher of this file that
// evaluates that head answers it here, before anything is enqueued (ww_k_crnn_ctc_forward below is its way in).  The zero-filled w1 / b1
// of its device block (model_pack.h) are the second line of defence, not the first.
int ww_crnn_refuse_ctc(ww_ctx *ctx, const ww_model *m, const char *what) {
  if (m && m->kind == WW_KIND_CRNN && m->crnn.HEAD == WW_HEAD_CTC)
    return ww_fail(ctx, WW_EINVAL, "%s: the model is a CTC-trained CRNN (per-step label posteriors, no wake-word posterior): it runs through "
                   "ww_ctc_forward, ww_ctc_forward_windows_dev and ww_ctc_slide_forward only", what);
  return WW_OK;
}

int ww_k_crnn_detect(ww_ctx *ctx, const ww_model *m, const float *d_enc, int nw, float *d_out) {
  if (int rc = ww_crnn_refuse_ctc(ctx, m, "ww_k_crnn_detect")) return rc;
  if (nw <= 0) return WW_OK;
  const ww_crnn_dev &c = m->crnn;
  if (!crnn_std_cell(c)) {
    ww_launch_scope scope(ctx, "crnn_head_kernel");
    hipLaunchKernelGGL(crnn_head_kernel, dim3(nw), dim3(64), 0, ctx->stream, d_enc, c.w1, c.b1, c.w2, c.b2, d_out, 2 * c.H, c.F, c.NOUT, c.HEAD);
    WW_HIP(ctx, hipGetLastError());
    return WW_OK;
  }
  ww_launch_scope scope(ctx, "crnn_detect_kernel");
  hipLaunchKernelGGL(crnn_detect_kernel, dim3(nw), dim3(64), 0, ctx->stream, d_enc, c.w1, c.b1, c.w2, c.b2, d_out, c.NOUT, c.HEAD);
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

// ------------------------------------------------------------------------------------------
// Generic geometry (ww_crnn_dev::generic): the older export the reference still ships
// (utils/CRNN_files/{encode,detect}_old.tflite - Conv2D 20x5 over freq x time, stride 8x2, VALID ->
// 74 steps of 3*32 features) and any other conv shape a retrained checkpoint may use.  Correctness path,
// not a tuned one: direct convolution on the vector ALU, the MFMA GEMM above on K padded to 64, one
// workgroup per window walking the recurrence with the step inputs read from global memory.
// ------------------------------------------------------------------------------------------
struct convg_args {
  const float *mel;
  win_addr wa;
  const float *wt;    // [KF*KT][C]
  const float *bias;  // [C]
  float *feat;        // [Nw][OT][FEATP]
  int n_mel, T, C, KF, KT, SF, ST, PF, PT, OF, OT, FEATP;
};

__global__ __launch_bounds__(256) void conv_generic_kernel(convg_args a) {
  extern __shared__ __align__(16) float cg_win[];  // [T][n_mel], rows >= valid zero
  const int tid = threadIdx.x, w = blockIdx.x;
  int64_t row;
  int valid;
  window_span(a.wa, w, a.T, row, valid);
  const float *src = a.mel + row * a.n_mel;
  for (int i = tid; i < a.T * a.n_mel; i += 256) cg_win[i] = i < valid * a.n_mel ? src[i] : 0.f;
  __syncthreads();
  float *dst = a.feat + (size_t)w * a.OT * a.FEATP;
  const int feat_w = a.OF * a.C;
  for (int o = tid; o < a.OT * a.FEATP; o += 256) {
    const int t = o / a.FEATP, col = o - t * a.FEATP;
    float v = 0.f;
    if (col < feat_w) {
      const int f = col / a.C, c = col - f * a.C;
      float acc = 0.f;
      for (int kf = 0; kf < a.KF; ++kf) {
        const int im = f * a.SF - a.PF + kf;
        if (im < 0 || im >= a.n_mel) continue;
        for (int kt = 0; kt < a.KT; ++kt) {
          const int it = t * a.ST - a.PT + kt;
          if (it < 0 || it >= a.T) continue;
          acc = fmaf(cg_win[it * a.n_mel + im], a.wt[(size_t)(kf * a.KT + kt) * a.C + c], acc);
        }
      }
      v = fmaxf(acc + a.bias[c], 0.f);
    }
    dst[o] = v;
  }
}

struct grug_args {
  const float *gx;   // [Nw][OT][2*3H] input projections incl. b_x
  const float *wh, *bh;
  float *seq;        // [Nw][OT][2H] (fwd | bwd) or nullptr
  float *last;       // [Nw][2H] (fwd_last | bwd_last) or nullptr
  int OT;
};

// wave 0 = forward, wave 1 = backward; the next step's three gate inputs are in flight while this step computes
__global__ __launch_bounds__(128) void gru_generic_kernel(grug_args a) {
  constexpr int H = GR_H;
  __shared__ __align__(16) float hbuf[2][2][H];
  const int tid = threadIdx.x, lane = tid & 63, dir = tid >> 6;
  const int unit = lane >> 1, half = lane & 1;
  const int w = blockIdx.x, OT = a.OT;
  gru_w g;
  gru_load_w(g, a.wh, a.bh, dir, unit, half);
  if (tid < 2 * H) hbuf[tid >> 5][0][tid & 31] = 0.f;
  __syncthreads();
  const float *gxl = a.gx + (size_t)w * OT * 6 * H + dir * 3 * H + unit;
  float h_own = 0.f;
  int t = dir ? OT - 1 : 0;
  float gz = gxl[(size_t)t * 6 * H], gr = gxl[(size_t)t * 6 * H + H], gc = gxl[(size_t)t * 6 * H + 2 * H];
  for (int s = 0; s < OT; ++s) {
    const int cur = s & 1;
    const int tn = dir ? t - 1 : t + 1;
    float nz = 0.f, nr = 0.f, nc = 0.f;
    if (s + 1 < OT) {
      nz = gxl[(size_t)tn * 6 * H]; nr = gxl[(size_t)tn * 6 * H + H]; nc = gxl[(size_t)tn * 6 * H + 2 * H];
    }
    float uz, ur, uc;
    h_own = gru_step<false>(g, &hbuf[dir][cur][0], half, gz, gr, gc, h_own, nullptr, uz, ur, uc);
    if (half == 0) {
      hbuf[dir][cur ^ 1][unit] = h_own;
      if (a.seq) a.seq[((size_t)w * OT + t) * 2 * H + dir * H + unit] = h_own;
    }
    wsync_h();
    gz = nz; gr = nr; gc = nc;
    t = tn;
  }
  if (a.last && half == 0) a.last[(size_t)w * 2 * H + dir * H + unit] = h_own;
}

// ------------------------------------------------------------------------------------------
// The cells the trainer's tuner can pick besides the shipped one (wwdetect/CRNN/train.py:112-125): a reset-after GRU or an LSTM of
// H = 16, 32, 48 or 64 units.  rnn_layer_kernel<CELL, H> is gru_generic_kernel's place in the layered path for them: one workgroup
// per window, both directions, gx [Nw][OT][2 G H] from the GEMM (G = 3 gate blocks z, r, h | 4 blocks i, f, c, o), the states to
// seq [Nw][OT][seq_ld] (forward | backward, then zeros up to seq_ld) and / or the last ones to last [Nw][2H].
//
// Lane map.  A direction is TPD threads, unit u = LPU lanes ("slices"), slice s holds the KS = H / LPU columns [s KS, (s + 1) KS) of
// the unit's G rows of W_h in registers (G KS floats: at most 128, LSTM of 64 units):
//     H    LPU  TPD  KS   waves per direction
//     16    4    64   4   1
//     32    2    64  16   1
//     48    2   128  24   2  (lanes 96..127 of a direction hold no unit: zero weights, no load, no store; their DPP partners are idle too)
//     64    2   128  32   2
// h ping-pongs through LDS.  A one-wave direction orders it with wsync_h (LDS traffic of one wave is served in issue order); a
// two-wave direction meets at lds_barrier() once per step - both directions run the same OT steps and no lane leaves the loop, so
// the workgroup barrier is uniform.  The next step's G projected inputs are in flight while this step computes.
//
// ONE association of a gate's pre-activation (gru_step's, extended to LPU slices): per slice s an even-k and an odd-k fmaf chain over
// the slice's columns, k ascending (the two halves of a packed fp32 FMA),
//     E_s: k = s KS, s KS + 2, ..      O_s: k = s KS + 1, s KS + 3, ..
// E_0 starts from the projected input x (from 0 for the GRU's candidate gate, whose x joins as tanh(x_c + r * hc)), O_0 from b_h (0
// for an LSTM, whose one bias is in x), every other chain from 0; a slice's value is E_s + O_s and the slices are joined by a fixed
// DPP tree: v += v[lane ^ 1], then for LPU = 4 v += v[lane ^ 2].  At (GRU, 32) this is (E0 + O0) + (E1 + O1), gru_step's bits.
// LSTM (Keras order i, f, c, o): c' = f c + i g, h' = o tanh(c') with g = tanh(pre_c), spelled out as gru_blend is.
// ------------------------------------------------------------------------------------------
template <int CELL, int H>
struct rnn_cfg {
  static_assert((CELL == WW_CELL_GRU || CELL == WW_CELL_LSTM) && (H == 16 || H == 32 || H == 48 || H == 64), "cells of 16, 32, 48, 64 units");
  static constexpr int G = CELL == WW_CELL_LSTM ? 4 : 3;
  static constexpr int LPU = H == 16 ? 4 : 2;
  static constexpr int TPD = H * LPU <= 64 ? 64 : 128;
  static constexpr int KS = H / LPU;
  static_assert(KS % 4 == 0 && H * LPU <= TPD && TPD % 64 == 0, "a slice is whole float4s; a direction is whole waves");
};

struct rnn_args {
  const float *gx;   // [Nw][OT][2*G*H] input projections incl. b_x
  const float *wh;   // [2][G*H][H]
  const float *bh;   // [2][G*H] (zeros for an LSTM)
  float *seq;        // [Nw][OT][seq_ld] (fwd | bwd | zeros) or nullptr
  float *last;       // [Nw][2H] (fwd_last | bwd_last) or nullptr
  int OT, seq_ld;
};

__device__ __forceinline__ float swap_quad2(float v) {
  // value of lane ^ 2: DPP quad_perm [2,3,0,1]
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));
}

__device__ __forceinline__ float lstm_cell(float i, float f, float g, float c) { return __fmaf_rn(f, c, __fmul_rn(i, g)); }
__device__ __forceinline__ float lstm_out(float o, float c) { return __fmul_rn(o, fast_tanh(c)); }

template <int CELL, int H>
__global__ __launch_bounds__((2 * rnn_cfg<CELL, H>::TPD)) void rnn_layer_kernel(rnn_args a) {
  using cfg = rnn_cfg<CELL, H>;
  constexpr int G = cfg::G, LPU = cfg::LPU, TPD = cfg::TPD, KS = cfg::KS, NQ = KS / 4, GX = 2 * G * H;
  __shared__ __align__(16) float hbuf[2][2][H];
  const int tid = threadIdx.x;
  const int dir = __builtin_amdgcn_readfirstlane(tid / TPD);  // (whole waves per direction)
  const int lt = tid - dir * TPD, unit = lt / LPU, slice = lt % LPU;
  const bool live = unit < H, own = live && slice == 0;  // own: the lane that carries the unit's state and stores it
  const int w = blockIdx.x, OT = a.OT;

  f32x2 wv[G][2 * NQ];
  float bh[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float *row = a.wh + ((size_t)dir * G * H + (size_t)g * H + (live ? unit : 0)) * H + slice * KS;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live) v = *(const float4 *)(row + 4 * q);
      wv[g][2 * q] = (f32x2){v.x, v.y};
      wv[g][2 * q + 1] = (f32x2){v.z, v.w};
    }
    bh[g] = own ? a.bh[dir * G * H + g * H + unit] : 0.f;  // slice 0's odd-k chain starts from b_h, every other one from zero
  }
  for (int i = tid; i < 2 * 2 * H; i += 2 * TPD) (&hbuf[0][0][0])[i] = 0.f;
  // the pad columns [2H, seq_ld) of every row, on every call: the next GEMM multiplies them by zero weights, and the workspace is
  // reused - 0 * NaN is NaN
  if (a.seq && a.seq_ld > 2 * H) {
    const int pad = a.seq_ld - 2 * H;
    for (int i = tid; i < OT * pad; i += 2 * TPD) {
      const int t = i / pad, col = i - t * pad;
      a.seq[((size_t)w * OT + t) * a.seq_ld + 2 * H + col] = 0.f;
    }
  }
  __syncthreads();

  const float *gxl = a.gx + (size_t)w * OT * GX + dir * G * H + (live ? unit : 0);
  int t = dir ? OT - 1 : 0;
  float x[G];
#pragma unroll
  for (int g = 0; g < G; ++g) x[g] = own ? gxl[(size_t)t * GX + g * H] : 0.f;
  float h_own = 0.f, c_own = 0.f;
  for (int s = 0; s < OT; ++s) {
    const int cur = s & 1;
    const int tn = dir ? t - 1 : t + 1;
    float nx[G];
#pragma unroll
    for (int g = 0; g < G; ++g) nx[g] = 0.f;
    if (own && s + 1 < OT) {
#pragma unroll
      for (int g = 0; g < G; ++g) nx[g] = gxl[(size_t)tn * GX + g * H];
    }
    const float4 *hp = (const float4 *)(&hbuf[dir][cur][slice * KS]);
    float4 hv[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) hv[q] = hp[q];
    f32x2 acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = (f32x2){(CELL == WW_CELL_GRU && g == 2) ? 0.f : x[g], bh[g]};  // (x and bh are 0 off slice 0)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const f32x2 h0 = {hv[q].x, hv[q].y}, h1 = {hv[q].z, hv[q].w};
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = __builtin_elementwise_fma(wv[g][2 * q], h0, acc[g]);
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = __builtin_elementwise_fma(wv[g][2 * q + 1], h1, acc[g]);
    }
    float pre[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float v = acc[g].x + acc[g].y;
      v += swap_pair(v);
      if (LPU == 4) v += swap_quad2(v);
      pre[g] = v;
    }
    if (CELL == WW_CELL_GRU) {
      const float z = fast_sigmoid(pre[0]), r = fast_sigmoid(pre[1]);
      h_own = gru_blend(z, h_own, gru_candidate(r, pre[2], x[2]));
    } else {
      const float ig = fast_sigmoid(pre[0]), fg = fast_sigmoid(pre[1]), gg = fast_tanh(pre[2]), og = fast_sigmoid(pre[G - 1]);
      c_own = lstm_cell(ig, fg, gg, c_own);
      h_own = lstm_out(og, c_own);
    }
    if (own) {
      hbuf[dir][cur ^ 1][unit] = h_own;
      if (a.seq) a.seq[((size_t)w * OT + t) * a.seq_ld + dir * H + unit] = h_own;
    }
    if (TPD == 64) wsync_h();
    else lds_barrier();
#pragma unroll
    for (int g = 0; g < G; ++g) x[g] = nx[g];
    t = tn;
  }
  if (a.last && own) a.last[(size_t)w * 2 * H + dir * H + unit] = h_own;
}

static int crnn_gates(const ww_crnn_dev &c) { return c.CELL == WW_CELL_LSTM ? 4 : 3; }

template <int CELL, int H>
static void launch_rnn_layer_as(ww_ctx *ctx, const rnn_args &a, int nw) {
  hipLaunchKernelGGL((rnn_layer_kernel<CELL, H>), dim3(nw), dim3(2 * rnn_cfg<CELL, H>::TPD), 0, ctx->stream, a);
}

static int launch_rnn_layer(ww_ctx *ctx, const ww_crnn_dev &c, const char *name, const rnn_args &a, int nw) {
  ww_launch_scope scope(ctx, name);
  switch (c.CELL * 100 + c.H) {
    case 16: launch_rnn_layer_as<WW_CELL_GRU, 16>(ctx, a, nw); break;
    case 32: launch_rnn_layer_as<WW_CELL_GRU, 32>(ctx, a, nw); break;
    case 48: launch_rnn_layer_as<WW_CELL_GRU, 48>(ctx, a, nw); break;
    case 64: launch_rnn_layer_as<WW_CELL_GRU, 64>(ctx, a, nw); break;
    case 116: launch_rnn_layer_as<WW_CELL_LSTM, 16>(ctx, a, nw); break;
    case 132: launch_rnn_layer_as<WW_CELL_LSTM, 32>(ctx, a, nw); break;
    case 148: launch_rnn_layer_as<WW_CELL_LSTM, 48>(ctx, a, nw); break;
    case 164: launch_rnn_layer_as<WW_CELL_LSTM, 64>(ctx, a, nw); break;
    default: return ww_fail(ctx, WW_EINTERNAL, "no recurrence kernel for cell %d of %d units (the loader should have refused it)", c.CELL, c.H);
  }
  return WW_OK;
}

static size_t crnn_generic_workspace(const ww_crnn_dev &c, int nw) {
  const size_t rows = (size_t)nw * c.OT;
  return ww_bump::need(rows * c.FEATP, 4) + ww_bump::need(rows * 2 * crnn_gates(c) * c.H, 4) + ww_bump::need(rows * c.SEQP, 4) +
         ww_bump::need((size_t)nw * 2 * c.H, 4) + 1024;
}

static void launch_gemm(ww_ctx *ctx, const char *name, const float *A, const float *W, const float *bias, float *C, int M, int N, int K) {
  const int n_tiles = (N + GB_N - 1) / GB_N, m_tiles = (M + GB_M - 1) / GB_M;
  gemm_args g = {A, W, bias, C, M, N, K, n_tiles};
  ww_launch_scope scope(ctx, name);
  // ids: 8 XCDs x (m-tiles of that residue, rounded up) x n-tiles; ids whose m-tile is past the end exit at once
  hipLaunchKernelGGL(gemm_nt_kernel, dim3(8 * ((m_tiles + 7) / 8) * n_tiles), dim3(512), 0, ctx->stream, g);
}

static int crnn_forward_generic(ww_ctx *ctx, const ww_model *m, const win_addr &wa, const float *d_mel, int nw, void *ws,
                                float *d_out, float *d_enc) {
  const ww_crnn_dev &c = m->crnn;
  const size_t rows = (size_t)nw * c.OT;
  ww_bump b(ws, ~size_t(0));
  const int GX = 2 * crnn_gates(c) * c.H;  // gate rows of both directions (6 H for a GRU)
  float *feat = b.take<float>(rows * c.FEATP), *gx = b.take<float>(rows * GX), *seq = b.take<float>(rows * c.SEQP);
  float *enc = b.take<float>((size_t)nw * 2 * c.H);
  if (d_enc) enc = d_enc;
  {
    convg_args a = {d_mel, wa, c.conv_wt, c.conv_b, feat, c.n_mel, c.T, c.C, c.KF, c.KT, c.SF, c.ST, c.PF, c.PT, c.OF, c.OT, c.FEATP};
    ww_launch_scope scope(ctx, "conv_generic_kernel");
    hipLaunchKernelGGL(conv_generic_kernel, dim3(nw), dim3(256), (size_t)c.T * c.n_mel * sizeof(float), ctx->stream, a);
  }
  launch_gemm(ctx, "gemm_nt_kernel<gru1,generic>", feat, c.wx1p, c.bx1, gx, (int)rows, GX, c.FEATP);
  if (!crnn_std_cell(c)) {
    // any cell but the shipped one: rnn_layer_kernel; layer 1's sequence has rows of SEQP (wx2 is packed to match: model_pack.h)
    const rnn_args a1 = {gx, c.wh1, c.bh1, seq, nullptr, c.OT, c.SEQP};
    if (int rc = launch_rnn_layer(ctx, c, "rnn_layer_kernel<seq>", a1, nw)) return rc;
    launch_gemm(ctx, "gemm_nt_kernel<gru2,generic>", seq, c.wx2, c.bx2, gx, (int)rows, GX, c.SEQP);
    const rnn_args a2 = {gx, c.wh2, c.bh2, nullptr, enc, c.OT, c.SEQP};
    if (int rc = launch_rnn_layer(ctx, c, "rnn_layer_kernel<last>", a2, nw)) return rc;
    WW_HIP(ctx, hipGetLastError());
    return ww_k_crnn_detect(ctx, m, enc, nw, d_out);
  }
  {
    grug_args a = {gx, c.wh1, c.bh1, seq, nullptr, c.OT};
    ww_launch_scope scope(ctx, "gru_generic_kernel<seq>");
    hipLaunchKernelGGL(gru_generic_kernel, dim3(nw), dim3(128), 0, ctx->stream, a);
  }
  launch_gemm(ctx, "gemm_nt_kernel<gru2,generic>", seq, c.wx2, c.bx2, gx, (int)rows, 6 * c.H, 2 * c.H);
  {
    grug_args a = {gx, c.wh2, c.bh2, nullptr, enc, c.OT};
    ww_launch_scope scope(ctx, "gru_generic_kernel<last>");
    hipLaunchKernelGGL(gru_generic_kernel, dim3(nw), dim3(128), 0, ctx->stream, a);
  }
  WW_HIP(ctx, hipGetLastError());
  return ww_k_crnn_detect(ctx, m, enc, nw, d_out);
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// Above this many windows per launch the recurrences move to gru_tail_kernel (one more kernel boundary and 14.6 KB per
// window through memory buy a CU-filling mix; below it one workgroup per window end to end is the shorter path).
// (ww_model_set_option(WW_OPT_CRNN_SPLIT_AT): 0 = always fused.)
static int crnn_split_threshold(const ww_model *m) { return m->opt_split_at; }

// Every CRNN kernel that asks for more than the default 64 KB of dynamic LDS.  The attribute is per device, so it is set
// for the device of every new context (ww_ctx_create, under its device scope) instead of once per process.
int ww_k_crnn_init_device(ww_ctx *ctx) {
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_stream_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_stream_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_stream_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_rows_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_rows_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_fused_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_FUSED_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_fused_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_FUSED_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_fused_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_FUSED_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_stream_kernel<0, true>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_stream_kernel<1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_stream_kernel<2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_stream_kernel<1, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_stream_kernel<2, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_stream_kernel<0, false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_stream_kernel<1, false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_stream_kernel<2, false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, CF_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_fused_bf16_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, CFB_SMEM_BYTES));
  WW_HIP(ctx, hipFuncSetAttribute((const void *)crnn_fused_bf16_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, CFB_SMEM_BYTES));
  return WW_OK;
}

// The arguments of the fused and streaming kernels: the model's weights, the launch's mel source, windows and outputs;
// gx_out and tag are left empty for the caller.
static fused_args crnn_fused_args(const ww_crnn_dev &c, const float *mel, const win_addr &wa, float *enc, float *out) {
  fused_args a = {};
  a.mel = mel; a.wa = wa;
  a.w4 = c.conv_w; a.cbias = c.conv_b;
  a.wx1s = c.wx1s; a.bx1 = c.bx1; a.wh1 = c.wh1; a.bh1 = c.bh1;
  a.wx2s = c.wx2s; a.bx2 = c.bx2; a.wh2 = c.wh2; a.bh2 = c.bh2;
  a.w1 = c.w1; a.b1 = c.b1; a.w2 = c.w2; a.b2 = c.b2;
  a.enc = enc; a.out = out;
  a.T = c.T; a.NOUT = c.NOUT; a.HEAD = c.HEAD;
  a.cwb = c.cwb; a.wx1b = c.wx1b;
  return a;
}

// streaming form (crnn_stream_kernel): standard geometry, fp32 contractions
bool ww_crnn_stream_capable(const ww_model *m) { return m->kind == WW_KIND_CRNN && !m->crnn.generic; }

// ONE launch per tick (crnn_stream_kernel<1 | 2>): 2 S workgroups, the posteriors as tags only.  every_k > 0 (a set bank that runs
// every_k member slots on every stream): 2 S every_k workgroups of the ALL form, set->ids a table of S every_k members
int ww_k_crnn_tick(ww_ctx *ctx, const ww_model *m, const ww_tick_fe &fe, int precise, float *d_gxc, const ww_tick_tag &tag,
                   const ww_set_ref *set, int every_k) {
  if (int rc = ww_crnn_refuse_ctc(ctx, m, "ww_k_crnn_tick")) return rc;
  const ww_crnn_dev &c = m->crnn;
  const ww_filter_dev &f = m->filt;
  if (c.generic || f.n_mel != CV_NMEL || fe.hop != 160)
    return ww_fail(ctx, WW_EINVAL, "one-launch streaming tick: standard conv geometry, 40 mel bands and hop 160 only");
  if (!tag.slots || fe.S <= 0) return ww_fail(ctx, WW_EINVAL, "one-launch streaming tick: no tag slots / no streams");
  stream_args sa = {};
  sa.f = crnn_fused_args(c, fe.hist, {nullptr, nullptr, 0, 0, 0, (int64_t)fe.S * fe.HR}, nullptr, nullptr);
  sa.f.tag = tag;
  sa.gxc = d_gxc;
  sa.fe = fe;
  sa.fb = ww_fe_filt_of(f);
  if (every_k < 0 || (every_k && !set) || (int64_t)fe.S * (every_k ? every_k : 1) > 65535)
    return ww_fail(ctx, WW_EINVAL, "one-launch streaming tick: %d member slots on %d streams", every_k, fe.S);
  const int nwg = 2 * fe.S * (every_k ? every_k : 1);
  {
    ww_launch_scope scope(ctx, "crnn_stream_kernel<tick>");
    if (every_k) {
      ww_set_all_ref all;
      all.ids = set->ids; all.aux = set->aux; all.stride = set->stride; all.K = every_k;
      if (precise) hipLaunchKernelGGL((crnn_stream_kernel<2, true, true>), dim3(nwg), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, sa, all);
      else hipLaunchKernelGGL((crnn_stream_kernel<1, true, true>), dim3(nwg), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, sa, all);
    } else if (set && precise) hipLaunchKernelGGL((crnn_stream_kernel<2, true>), dim3(nwg), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, sa, *set);
    else if (set) hipLaunchKernelGGL((crnn_stream_kernel<1, true>), dim3(nwg), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, sa, *set);
    else if (precise) hipLaunchKernelGGL(crnn_stream_kernel<2>, dim3(nwg), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, sa, ww_set_ref{});
    else hipLaunchKernelGGL(crnn_stream_kernel<1>, dim3(nwg), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, sa, ww_set_ref{});
  }
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

int ww_k_crnn_stream_forward(ww_ctx *ctx, const ww_model *m, const float *d_hist, int64_t hist_rows, const int64_t *d_win_row,
                             const int32_t *d_win_valid, const int32_t *d_win_aux, float *d_gxc, int nw, float *d_out,
                             const ww_tick_tag *tag, const ww_set_ref *set) {
  if (int rc = ww_crnn_refuse_ctc(ctx, m, "ww_k_crnn_stream_forward")) return rc;
  if (nw <= 0) return WW_OK;
  const ww_crnn_dev &c = m->crnn;
  if (c.generic) return ww_fail(ctx, WW_EINVAL, "streaming CRNN kernel: standard conv geometry only");
  if (!d_win_row || !d_win_valid || !d_win_aux) return ww_fail(ctx, WW_EINVAL, "streaming CRNN kernel: NULL window table");
  stream_args sa = {};
  sa.f = crnn_fused_args(c, d_hist, {d_win_row, d_win_valid, 0, 0, 0, hist_rows}, nullptr, d_out);
  sa.aux = d_win_aux;
  sa.gxc = d_gxc;
  if (tag) sa.f.tag = *tag;
  {
    ww_launch_scope scope(ctx, "crnn_stream_kernel");
    if (set) hipLaunchKernelGGL((crnn_stream_kernel<0, true>), dim3(nw), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, sa, *set);
    else hipLaunchKernelGGL(crnn_stream_kernel<0>, dim3(nw), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, sa, ww_set_ref{});
  }
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

// Everything behind the layer-1 projections: sixteen windows per workgroup with the recurrent products on the matrix pipe
// (gru_tail16_kernel), or one window per workgroup on the vector ALU (gru_tail_kernel).  The matrix form is a 38-step serial
// chain of ~4 k cycles per step on two waves: it needs >= ~600 workgroups to beat the vector form (tools/tail_sweep.py:
// front + tail per launch 743 vs 745 us at 9,216 windows, 1,204 vs 1,309 at 16,384, but 226 vs 188 at 2,048), so
// WW_OPT_CRNN_TAIL_MFMA = 1 (default) takes it from WW_TAIL16_MIN windows per launch on; 2 = always, 0 = never.
#define WW_TAIL16_MIN 9216
static size_t tail_seq_bytes(int nw) { return ww_bump::need((size_t)((nw + 15) / 16) * CV_OT * 16 * 2 * GR_H, 4); }
// The tail kernels' arguments: the model's weights; the caller names its source of projected rows (gx1, or gxI / gxL / gxR with
// hop_g, eight_g and, for several sequences, iI0) and its outputs (enc, out).
static tail_args crnn_tail_args(const ww_crnn_dev &c) {
  tail_args t = {};
  t.wh1 = c.wh1; t.bh1 = c.bh1;
  t.wx2s = c.wx2s; t.wx2 = c.wx2; t.bx2 = c.bx2; t.wh2 = c.wh2; t.bh2 = c.bh2;
  t.w1 = c.w1; t.b1 = c.b1; t.w2 = c.w2; t.b2 = c.b2;
  t.NOUT = c.NOUT; t.HEAD = c.HEAD;
  return t;
}
// set / slots: a model set's launch (the SET kernels, `slots` planes of nw windows each: seq holds slots x tail_seq_bytes(nw))
static void launch_tail(ww_ctx *ctx, const ww_model *m, const tail_args &t, int nw, float *seq, const ww_set_ref *set = nullptr, int slots = 1) {
  if (m->opt_tail_mfma >= 2 || (m->opt_tail_mfma == 1 && nw >= WW_TAIL16_MIN)) {
    tail16_args a16 = {t, seq, nw};
    ww_launch_scope scope(ctx, set ? "gru_tail16_kernel<set>" : "gru_tail16_kernel");
    const unsigned groups = (unsigned)((nw + 15) / 16);
    if (set) hipLaunchKernelGGL(gru_tail16_kernel<true>, dim3(groups, (unsigned)slots), dim3(128), GT16_SMEM_BYTES, ctx->stream, a16, *set);
    else hipLaunchKernelGGL(gru_tail16_kernel<false>, dim3(groups), dim3(128), GT16_SMEM_BYTES, ctx->stream, a16, ww_set_ref{});
  } else {
    ww_launch_scope scope(ctx, set ? "gru_tail_kernel<set>" : "gru_tail_kernel");
    if (set) hipLaunchKernelGGL(gru_tail_kernel<true>, dim3((unsigned)nw, (unsigned)slots), dim3(128), 0, ctx->stream, t, *set);
    else hipLaunchKernelGGL(gru_tail_kernel<false>, dim3((unsigned)nw), dim3(128), 0, ctx->stream, t, ww_set_ref{});
  }
}

// Regular sliding windows (hop <= 8 over one mel sequence, every window complete) take crnn_rows_kernel + gru_tail_kernel from
// this many windows on (ww_model_set_option(WW_OPT_CRNN_SLIDE_MIN): 0 = never).
static int crnn_slide_min(const ww_model *m) { return m->opt_slide_min > 0 ? m->opt_slide_min : 0x7fffffff; }

// crnn_rows_kernel's arguments but for its position lists (start / stride / count / tiles, or desc): the three output lists are
// interior fields, left edges, right edges
static rows_args rows_args_of(const ww_crnn_dev &c, const float *mel, int64_t mel_rows, float *gI, float *gL, float *gR) {
  rows_args r = {};
  r.mel = mel; r.mel_rows = mel_rows;
  r.w4[0] = c.conv_w; r.w4[1] = c.conv_wL; r.w4[2] = c.conv_wR;
  r.cbias = c.conv_b; r.wx1s = c.wx1s; r.bx1 = c.bx1;
  r.out[0] = gI; r.out[1] = gL; r.out[2] = gR;
  return r;
}
// set / slots: as launch_tail's (the three output lists hold `slots` planes each)
static void launch_rows(ww_ctx *ctx, const rows_args &r, unsigned tiles, const ww_set_ref *set = nullptr, int slots = 1) {
  ww_launch_scope scope(ctx, set ? "crnn_rows_kernel<set>" : "crnn_rows_kernel");
  if (set) hipLaunchKernelGGL(crnn_rows_kernel<true>, dim3(tiles, (unsigned)slots), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, r, *set);
  else hipLaunchKernelGGL(crnn_rows_kernel<false>, dim3(tiles), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, r, ww_set_ref{});
}

// Scratch of a launch of nw windows, for sizing a buffer (ww_crnn_workspace) and for checking the one handed in
// (ww_k_crnn_forward).  Sliding form: (fields + 2 edge rows per window) x 192 floats; fields <= 7 nw + 130 (hop 7), i.e. never
// more than the 19 rows per window of the front + tail form.
static size_t crnn_slide_scratch(int nw) { return ww_bump::need(((size_t)9 * nw + 160) * 6 * GR_H, 4) + tail_seq_bytes(nw) + 2048; }
static size_t crnn_split_scratch(const ww_crnn_dev &c, int nw) {
  return ww_bump::need((size_t)nw * c.OT * 6 * c.H, 4) + tail_seq_bytes(nw) + 2048;
}

// Several mel sequences in one buffer (the clips of a test set, wwhip/evaluate.py), each slid over with the same hop:
// crnn_rows_kernel by tile descriptors (no tile straddles two sequences), gru_tail_kernel with each window's first
// interior field given explicitly.  seg_row0 / seg_nw are HOST arrays; windows are numbered sequence by sequence.
// sc: a model set's call (ww_set_forward_segments_dev; m is the set's view, sc->ids the call's member slots on the HOST, already
// checked).  Every group is then ONE crnn_rows_kernel<SET> launch and ONE tail launch over a (tiles | windows | groups of sixteen) x
// n_ids grid.  A group's tile table and i0 are built and uploaded once and serve every slot; the projected-row lists, the tail16
// scratch and the output are member-major planes: d_out is [n_ids][W][NOUT], W = the call's windows per member.  Groups stay whole
// sequences with n_ids x nW <= WW_SEG_GROUP (a single larger sequence is a group of its own), so the workspace bound is one model's.
bool ww_crnn_segments_capable(const ww_model *m, int hop) {
  return m->kind == WW_KIND_CRNN && !m->crnn.generic && hop >= 1 && hop <= 8 &&
         crnn_slide_min(m) != 0x7fffffff;
}
bool ww_crnn_set_segments_rows_form(const ww_model *m, int hop, int64_t W) { return ww_crnn_segments_capable(m, hop) && W >= crnn_slide_min(m); }

int ww_k_crnn_segments_forward(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *seg_row0,
                               const int32_t *seg_nw, int n_seg, int hop, float *d_out, const ww_crnn_set_call *sc) {
  if (int rc = ww_crnn_refuse_ctc(ctx, m, "ww_k_crnn_segments_forward")) return rc;
  const ww_crnn_dev &c = m->crnn;
  const int g = crnn_gcd8(hop), n_ids = sc ? sc->n_ids : 1;
  const int64_t cap = sc ? std::max<int64_t>(WW_SEG_GROUP / n_ids, 1) : WW_SEG_GROUP;
  crnn_seg_group gp;  // launch_plan.h: groups of whole sequences of at most ~WW_SEG_GROUP windows x slots bound the workspace
  int64_t w_done = 0;
  for (int s0 = 0; s0 < n_seg; s0 = gp.next) {
    if (int rc = crnn_plan_group(seg_row0, seg_nw, n_seg, hop, c.T, c.PT, c.OT, c.ST, mel_rows, s0, gp, cap)) return ww_fail(ctx, rc, "%s", gp.err);
    const int64_t nI = gp.nI, nW = gp.nW;
    if (nW > 0) {
      const int32_t aux[WW_SLIDE_AUX_N] = {(int32_t)nI, (int32_t)nW, (int32_t)(sc ? sc->W : 0), 0};
      ww_tables tb;
      const size_t o_tiles = tb.add(gp.tiles), o_i0 = tb.add(gp.i0);
      const size_t o_ids = sc ? tb.add(sc->ids, (size_t)n_ids) : 0, o_aux = sc ? tb.add(aux, (size_t)WW_SLIDE_AUX_N) : 0;
      const size_t b_seq = tail_seq_bytes((int)nW) * (size_t)n_ids;
      int rc = ww_ensure(ctx, ctx->dev, tb.bytes() + 3 * 256 + (size_t)n_ids * (size_t)(nI + 2 * nW) * 6 * c.H * 4 + b_seq + 8192, false);
      if (rc) return rc;
      ww_bump b(ctx->dev.ptr, ctx->dev.cap);
      char *d_tab = b.take<char>(tb.bytes());
      float *gI = b.take<float>((size_t)n_ids * nI * 6 * c.H), *gL = b.take<float>((size_t)n_ids * nW * 6 * c.H);
      float *gR = b.take<float>((size_t)n_ids * nW * 6 * c.H);
      float *seq = (float *)b.take<char>(b_seq);
      // the call goes on to build the next group (or returns) while this group's kernels run
      if ((rc = tb.send(ctx, d_tab))) return rc;
      ww_set_ref ref;
      if (sc) {
        ref.ids = (const int32_t *)(d_tab + o_ids);
        ref.aux = (const int32_t *)(d_tab + o_aux);
        ref.stride = sc->stride;
      }
      const ww_set_ref *set = sc ? &ref : nullptr;
      rows_args r = rows_args_of(c, d_mel, mel_rows, gI, gL, gR);
      r.desc = (const rows_tile *)(d_tab + o_tiles);
      launch_rows(ctx, r, (unsigned)gp.tiles.size(), set, n_ids);
      tail_args t = crnn_tail_args(c);
      t.gxI = gI; t.gxL = gL; t.gxR = gR;
      t.hop_g = hop / g; t.eight_g = 8 / g; t.iI0 = (const int64_t *)(d_tab + o_i0);
      t.out = d_out + (size_t)w_done * c.NOUT;
      launch_tail(ctx, m, t, (int)nW, seq, set, n_ids);
      WW_HIP(ctx, hipGetLastError());
      w_done += nW;
    }
  }
  return WW_OK;
}

size_t ww_crnn_workspace(const ww_model *m, int nw, bool sliding) {
  const ww_crnn_dev &c = m->crnn;
  if (c.generic) return crnn_generic_workspace(c, nw);
  const int thr = crnn_split_threshold(m);
  size_t need = 1024;  // crnn_fused_kernel keeps every intermediate in LDS
  if (sliding && nw >= crnn_slide_min(m)) need = crnn_slide_scratch(nw);
  if (thr > 0 && nw > thr) need = std::max(need, crnn_split_scratch(c, nw));
  return need;
}

// the one-kernel forms write a tick's tags (cf_phases_d_to_g); the front + tail forms and the generic path do not
bool ww_crnn_forward_tags(const ww_model *m, int nw) {
  return !m->crnn.generic && !(crnn_split_threshold(m) > 0 && nw > crnn_split_threshold(m));
}

int ww_k_crnn_forward(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                      const int32_t *d_win_valid, int64_t row0, int hop, int valid_const, int nw, void *ws, size_t ws_bytes,
                      float *d_out, float *d_enc, const ww_tick_tag *tag, const ww_set_ref *set) {
  if (int rc = ww_crnn_refuse_ctc(ctx, m, "ww_k_crnn_forward")) return rc;
  if (nw <= 0) return WW_OK;
  const ww_crnn_dev &c = m->crnn;
  win_addr wa = {d_win_row, d_win_valid, row0, hop, valid_const, mel_rows};
  if (set) {
    // a model set's explicit windows (m is the set's view: member 0's arguments, which each workgroup moves on to its own member):
    // crnn_fused_kernel<false, SET> in ONE launch whatever nw is - no scratch, no sliding form, no front + tail split, no bf16
    if (c.generic) return ww_fail(ctx, WW_EINVAL, "model set: standard conv geometry only");
    const fused_args a = crnn_fused_args(c, d_mel, wa, d_enc, d_out);
    {
      ww_launch_scope scope(ctx, "crnn_fused_kernel<set>");
      hipLaunchKernelGGL((crnn_fused_kernel<false, true>), dim3(nw), dim3(CF_THREADS), CF_FUSED_SMEM_BYTES, ctx->stream, a, *set);
    }
    WW_HIP(ctx, hipGetLastError());
    return WW_OK;
  }
  // the scratch this launch takes under the model's CURRENT options (ww_model_set_option may have moved the thresholds
  // since the caller sized ws): never past the end of what was handed in
  const bool slide_form = !c.generic && !d_win_row && !d_win_valid && valid_const >= c.T && hop >= 1 && hop <= 8 && nw >= crnn_slide_min(m) &&
                          row0 >= 0 && row0 + (int64_t)(nw - 1) * hop + c.T <= mel_rows;
  {
    size_t need = 0;
    if (c.generic) need = crnn_generic_workspace(c, nw);
    else if (slide_form) need = crnn_slide_scratch(nw);
    else if (crnn_split_threshold(m) > 0 && nw > crnn_split_threshold(m)) need = crnn_split_scratch(c, nw);
    if (need > ws_bytes)
      return ww_fail(ctx, WW_EINVAL, "CRNN launch of %d windows needs %zu bytes of scratch, the caller reserved %zu (options changed "
                     "after the buffer was sized?)", nw, need, ws_bytes);
  }
  if (c.generic && tag && tag->slots) return ww_fail(ctx, WW_EINVAL, "tick tags: the generic CRNN path does not write them");
  if (c.generic) return crnn_forward_generic(ctx, m, wa, d_mel, nw, ws, d_out, d_enc);
  fused_args a = crnn_fused_args(c, d_mel, wa, d_enc, d_out);
  const bool bf16 = m->precision == WW_PRECISION_BF16X3;
  // (also in split-bf16 mode: the mode permits bf16 products, and computing a seventh of them in fp32 is both faster and closer)
  if (slide_form) {
    // windows sliding over one sequence: 1 + 2 positions per window instead of 19 (crnn_rows_kernel)
    const int g = crnn_gcd8(hop);
    const int64_t n_int = crnn_n_int(nw, hop);
    ww_bump b(ws, ws_bytes);
    float *gI = b.take<float>((size_t)n_int * 6 * c.H), *gL = b.take<float>((size_t)nw * 6 * c.H), *gR = b.take<float>((size_t)nw * 6 * c.H);
    float *seq = (float *)b.take<char>(tail_seq_bytes(nw));
    rows_args r = rows_args_of(c, d_mel, mel_rows, gI, gL, gR);
    r.start[0] = row0 + 2; r.start[1] = row0 - c.PT; r.start[2] = row0 + (int64_t)(c.OT - 1) * c.ST - c.PT;
    r.stride[0] = g; r.stride[1] = hop; r.stride[2] = hop;
    r.count[0] = (int)n_int; r.count[1] = nw; r.count[2] = nw;
    for (int k = 0; k < 3; ++k) r.tiles[k] = (r.count[k] + 15) / 16;
    launch_rows(ctx, r, (unsigned)(r.tiles[0] + r.tiles[1] + r.tiles[2]));
    tail_args t = crnn_tail_args(c);
    t.gxI = gI; t.gxL = gL; t.gxR = gR;
    t.hop_g = hop / g; t.eight_g = 8 / g;
    t.enc = d_enc; t.out = d_out;
    launch_tail(ctx, m, t, nw, seq);
    WW_HIP(ctx, hipGetLastError());
    return WW_OK;
  }
  const int thr = crnn_split_threshold(m);
  if (tag && tag->slots) {
    if (slide_form || (thr > 0 && nw > thr)) return ww_fail(ctx, WW_EINVAL, "tick tags: this launch form does not write them");
    a.tag = *tag;
  }
  if (thr > 0 && nw > thr) {
    ww_bump b(ws, ws_bytes);
    a.gx_out = b.take<float>((size_t)nw * c.OT * 6 * c.H);
    float *seq = (float *)b.take<char>(tail_seq_bytes(nw));
    {
      ww_launch_scope scope(ctx, bf16 ? "crnn_fused_kernel<front,bf16x3>" : "crnn_fused_kernel<front>");
      if (bf16) hipLaunchKernelGGL(crnn_fused_bf16_kernel<true>, dim3(nw), dim3(CF_THREADS), CFB_SMEM_BYTES, ctx->stream, a);
      else hipLaunchKernelGGL(crnn_fused_kernel<true>, dim3(nw), dim3(CF_THREADS), CF_FUSED_SMEM_BYTES, ctx->stream, a, ww_set_ref{});
    }
    tail_args t = crnn_tail_args(c);
    t.gx1 = a.gx_out;
    t.enc = d_enc; t.out = d_out;
    launch_tail(ctx, m, t, nw, seq);
    WW_HIP(ctx, hipGetLastError());
    return WW_OK;
  }
  {
    ww_launch_scope scope(ctx, bf16 ? "crnn_fused_kernel<bf16x3>" : "crnn_fused_kernel");
    if (bf16) hipLaunchKernelGGL(crnn_fused_bf16_kernel<false>, dim3(nw), dim3(CF_THREADS), CFB_SMEM_BYTES, ctx->stream, a);
    else hipLaunchKernelGGL(crnn_fused_kernel<false>, dim3(nw), dim3(CF_THREADS), CF_FUSED_SMEM_BYTES, ctx->stream, a, ww_set_ref{});
  }
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

// ------------------------------------------------------------------------------------------
// A CTC-trained CRNN's launches: always crnn_fused_kernel<front> (fp32), then gru_tail_ctc_kernel - for sliding windows too, whatever
// WW_OPT_CRNN_SLIDE_MIN says.  crnn_rows_kernel's projected rows are not the front kernel's bits (it deals every position to a
// 16-row MFMA tile, the front kernel rows 16..18 of a window to 4x4x1 blocks whose partial sums meet at the end: the posteriors of
// the two forms differ by up to 4e-7, and tests/test_gpu_parity.py allows the other heads 2e-6 there).  A decoded label is an argmax:
// a window must read the same whether it arrives in a list or under a hop, so there is ONE front.
// ------------------------------------------------------------------------------------------
int ww_crnn_ctc_check(ww_ctx *ctx, const ww_model *m, const char *what) {
  if (m->kind != WW_KIND_CRNN || m->crnn.HEAD != WW_HEAD_CTC)
    return ww_fail(ctx, WW_EINVAL, "%s: the model is not a CTC-trained CRNN (WW_HEAD_CTC); ww_forward and its family run it", what);
  if (m->crnn.generic || m->crnn.H != GR_H || m->crnn.OT != CV_OT || m->crnn.NOUT < 2 || m->crnn.NOUT > 8)
    return ww_fail(ctx, WW_EINTERNAL, "%s: a CTC model of a geometry the loader should have refused", what);
  if (m->precision != WW_PRECISION_FP32) return ww_fail(ctx, WW_EINVAL, "%s: a CTC-trained CRNN runs in WW_PRECISION_FP32 only", what);
  return WW_OK;
}

// scratch of a launch of nw >= 1 windows (the projected rows; the model's options do not move it)
size_t ww_crnn_ctc_workspace(const ww_model *m, int nw) { return ww_bump::need((size_t)nw * m->crnn.OT * 6 * m->crnn.H, 4) + 2048; }

int ww_k_crnn_ctc_forward(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                          const int32_t *d_win_valid, int64_t row0, int hop, int valid_const, int nw, void *ws, size_t ws_bytes,
                          int max_labels, int32_t *d_labels, int32_t *d_lengths, float *d_steps, float *d_enc) {
  if (int rc = ww_crnn_ctc_check(ctx, m, "ww_k_crnn_ctc_forward")) return rc;
  if (max_labels < 1 || max_labels > CV_OT || !d_labels || !d_lengths) return ww_fail(ctx, WW_EINVAL, "CTC launch: max_labels %d / NULL output", max_labels);
  if (nw <= 0) return WW_OK;
  const ww_crnn_dev &c = m->crnn;
  const size_t need = ww_crnn_ctc_workspace(m, nw);
  if (need > ws_bytes) return ww_fail(ctx, WW_EINVAL, "CTC launch of %d windows needs %zu bytes of scratch, the caller reserved %zu", nw, need, ws_bytes);
  const win_addr wa = {d_win_row, d_win_valid, row0, hop, valid_const, mel_rows};
  fused_args a = crnn_fused_args(c, d_mel, wa, nullptr, nullptr);
  ww_bump b(ws, ws_bytes);
  a.gx_out = b.take<float>((size_t)nw * c.OT * 6 * c.H);
  {
    ww_launch_scope scope(ctx, "crnn_fused_kernel<front>");
    hipLaunchKernelGGL(crnn_fused_kernel<true>, dim3(nw), dim3(CF_THREADS), CF_FUSED_SMEM_BYTES, ctx->stream, a, ww_set_ref{});
  }
  tail_ctc_args ca = {};
  ca.t = crnn_tail_args(c);
  ca.t.gx1 = a.gx_out;
  ca.t.enc = d_enc;
  ca.steps = d_steps; ca.labels = d_labels; ca.lengths = d_lengths; ca.max_labels = max_labels;
  {
    ww_launch_scope scope(ctx, "gru_tail_ctc_kernel");
    hipLaunchKernelGGL(gru_tail_ctc_kernel, dim3((unsigned)nw), dim3(128), 0, ctx->stream, ca);
  }
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

int ww_k_ctc_greedy(ww_ctx *ctx, const float *d_steps, int64_t n, int T, int L, int max_labels, int32_t *d_labels, int32_t *d_lengths) {
  if (n <= 0) return WW_OK;
  {
    ww_launch_scope scope(ctx, "ctc_greedy_kernel");
    hipLaunchKernelGGL(ctc_greedy_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_steps, (long long)n, T, L, max_labels,
                       d_labels, d_lengths);
  }
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

// A CTC stream bank's incremental ticks: ww_k_crnn_tick and ww_k_crnn_stream_forward for crnn_stream_kernel's CTC form.  The same
// launch geometry and arguments; a window's decode leaves as one word (stream_ctc.h), its posteriors on request to d_steps.
int ww_k_crnn_ctc_tick(ww_ctx *ctx, const ww_model *m, const ww_tick_fe &fe, int precise, float *d_gxc, const ww_tick_tag &tag, float *d_steps) {
  if (int rc = ww_crnn_ctc_check(ctx, m, "ww_k_crnn_ctc_tick")) return rc;
  const ww_crnn_dev &c = m->crnn;
  const ww_filter_dev &f = m->filt;
  if (f.n_mel != CV_NMEL || fe.hop != 160) return ww_fail(ctx, WW_EINVAL, "one-launch streaming tick: standard conv geometry, 40 mel bands and hop 160 only");
  if (!tag.slots || fe.S <= 0 || fe.S > 65535) return ww_fail(ctx, WW_EINVAL, "one-launch streaming tick: no tag slots / %d streams", fe.S);
  stream_args sa = {};
  sa.f = crnn_fused_args(c, fe.hist, {nullptr, nullptr, 0, 0, 0, (int64_t)fe.S * fe.HR}, nullptr, nullptr);
  sa.f.tag = tag;
  sa.gxc = d_gxc;
  sa.fe = fe;
  sa.fb = ww_fe_filt_of(f);
  {
    ww_launch_scope scope(ctx, "crnn_stream_kernel<tick,ctc>");
    if (precise) hipLaunchKernelGGL((crnn_stream_kernel<2, false, false, true>), dim3(2 * fe.S), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, sa, ww_ctc_ref{d_steps});
    else hipLaunchKernelGGL((crnn_stream_kernel<1, false, false, true>), dim3(2 * fe.S), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, sa, ww_ctc_ref{d_steps});
  }
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

int ww_k_crnn_ctc_stream_forward(ww_ctx *ctx, const ww_model *m, const float *d_hist, int64_t hist_rows, const int64_t *d_win_row,
                                 const int32_t *d_win_valid, const int32_t *d_win_aux, float *d_gxc, int nw, uint32_t *d_words, float *d_steps,
                                 const ww_tick_tag *tag) {
  if (int rc = ww_crnn_ctc_check(ctx, m, "ww_k_crnn_ctc_stream_forward")) return rc;
  if (nw <= 0) return WW_OK;
  const ww_crnn_dev &c = m->crnn;
  if (!d_win_row || !d_win_valid || !d_win_aux) return ww_fail(ctx, WW_EINVAL, "streaming CRNN kernel: NULL window table");
  if (!d_words && !(tag && tag->slots)) return ww_fail(ctx, WW_EINVAL, "streaming CTC kernel: neither an output block nor tag slots");
  stream_args sa = {};
  sa.f = crnn_fused_args(c, d_hist, {d_win_row, d_win_valid, 0, 0, 0, hist_rows}, nullptr, (float *)d_words);  // (words: cf_phases_d_to_g_ctc)
  sa.aux = d_win_aux;
  sa.gxc = d_gxc;
  if (tag) sa.f.tag = *tag;
  {
    ww_launch_scope scope(ctx, "crnn_stream_kernel<ctc>");
    hipLaunchKernelGGL((crnn_stream_kernel<0, false, false, true>), dim3(nw), dim3(CF_THREADS), CF_SMEM_BYTES, ctx->stream, sa, ww_ctc_ref{d_steps});
  }
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}
