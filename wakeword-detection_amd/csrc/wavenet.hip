// Wavenet encode + detect for gfx950 (fp32 MFMA, one persistent workgroup per window).
//
// Replaces encode.tflite + detect.tflite of the reference Wavenet (tf_lite_models/Wavenet;
// architecture wwdetect/wavenet/wavenet_model.py:11-128; call sites
// spokestack/wakeword/tflite.py:205-231, utils/evaluate_models.py:83-86).
//
// A 768-thread workgroup (12 wavefronts, 3 per SIMD) walks all 24 gated residual blocks of one
// 182x40 window without leaving the CU.  Time is the MFMA M dimension: 182 -> 12 tiles of 16
// rows, one tile per wave.  Two arithmetic modes (ww_model_set_precision):
//
// fp32 (default): v_mfma_f32_16x16x4_f32.  The residual stream x[182][16] and the skip accumulator
// [182][32] never leave registers: they sit in the accumulator layout (lane -> column, 4 rows per
// register quad), which is also the layout the next block's epilogue needs.  Only the BatchNorm
// output u (which the dilated taps of OTHER rows read) and the gate product g (D-layout ->
// A-layout transpose) go through LDS:
//     u = x*s + t                      -> LDS (double buffered, 16 zero rows in front = causal pad)
//     [sig|tanh] = u[t-(2-k)d] * Wg    3 taps x 16 ch = K 48, N 32     24 MFMA / 16 rows
//     g = tanh(.)*sigmoid(.)           -> LDS (wave-private tile)
//     [res|skip] = g * Wrs             K 16, N 48                      12 MFMA / 16 rows
//     x += relu(res); skip += relu(skip_b)
// One __syncthreads per block.  On gfx950 the fp32 MFMA shares the SIMD's fp32 datapath with the
// vector ALU, so MFMA and VALU time add up (ablations: dropping the 24 gate MFMAs saves exactly their
// 21.7 us of 77; dropping the gate transcendentals or the barrier saves < 1 us; hand-interleaving
// VALU into one wave's MFMA gaps made it slower): the kernel runs at ~86 % of that sum.
//
// split-bf16 ("bf16x3"): see the block before the kernel - transposed block loop on
// v_mfma_f32_16x16x32_bf16, operands straight from registers, parameters through LDS pages.
//
// The detect head (ReLU, 1x1 32->32 ReLU, 1x1 32->2, max over time, softmax) runs in the same launch.
//
// wavenet_seq_kernel (fp32): the same block loop over a mel sequence of ANY length - the model as its trainer builds it with
// timesteps=None, causal zeros in front of row 0 only - walked in chunks with each block's last 16 rows of u carried from chunk
// to chunk; whole sequences (ww_wave_sequence) and, one wave per stream, a causal bank's tick (WW_STREAM_CAUSAL).  See there.
#include "stream_fe.h"
#undef NB   // (fft_device.h: bins of the transform; here NB is the model's block count)
#undef WIN

#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define WV_T 192      // padded time (12 tiles of 16)
#define WV_C 16
#define WV_S 32
#define WV_PAD 16     // causal zero rows in front of u
#define WV_INLD 48    // staged input row stride (40 mel + zero pad to 3 k-blocks)
// wavefronts per workgroup = template parameter NW of the kernel: the 12 row tiles of 16 frames are dealt 12 / NW per wave.
// Both modes run 12 waves x 1 tile (3 waves per SIMD).  The split-bf16 loop is written over the tiles of a wave; its 6- and
// 4-wave forms (2 and 3 tiles per wave: independent MFMAs / gate evaluations back to back in one wave, a third of the operand
// reads) measured 45.2 and 44.6 us against 38.9 us for 12 x 1 - a wave's LDS and MFMA -> VALU latencies are covered better
// by two more waves on the SIMD than by two more tiles in the wave.
#ifndef WV_F32_WIDE_FROM
#define WV_F32_WIDE_FROM 256   // the fp32 transposed loop likewise (round 5)
#endif
#ifndef WV_BF16_WIDE_FROM
#define WV_BF16_WIDE_FROM 256  // launches of more windows than this (= CUs of the chip) take the 4-wave x 3-tile form, two workgroups per CU
#endif
#ifndef WV_BF16_OCC
#define WV_BF16_OCC 3   // waves per SIMD the split-bf16 kernel is compiled for (3 = one workgroup per CU)
#endif

struct win_addr_w {
  const int64_t *row;
  const int32_t *valid;
  int64_t row0;
  int hop;
  int valid_const;
  int64_t mel_rows;
};

struct wave_args {
  const float *mel;
  win_addr_w wa;
  int T, n_mel, NB, NOUT;
  unsigned long long dil4[2];  // dilation of block b: 4 bits at bit 4*(b%16) of dil4[b/16]  (d <= 8, NB <= 32)
  unsigned int has_res_mask;   // bit b: block b has a residual 1x1 conv
  const float *w_in4;   // [3 kb][4 kk][16 col][4 q]   (K = 40 padded to 48)
  const float *b_in;    // [16]
  const float *bn_s, *bn_t;  // [NB][16]
  const float *w_gate4; // [NB][3 kb][4 kk][32 col][4 q]
  const float *b_gate;  // [NB][32]  (sig | tanh)
  const float *w_rs4;   // [NB][4 kk][48 col][4 q]
  const float *b_rs;    // [NB][48]  (res | skip)
  const float *d_w1_4;  // [2 kb][4 kk][32 col][4 q]
  const float *d_b1;    // [32]
  const float *d_w2_4;  // [2 kb][4 kk][16 col][4 q]  (NOUT padded to 16)
  const float *d_b2;    // [16]
  float *out;           // [Nw][NOUT]
  float *enc;           // optional [Nw][T][32]
  const float *enc_in;  // HEAD_ONLY: encoder output to run the detect graph on
  const uint4 *wpk;     // split-bf16 mode: parameter pages [NB][WV_PAGE_U4] (A operands of v_mfma_f32_16x16x32_bf16, then the vectors)
  ww_tick_tag tag;      // streaming ticks: the posterior as a {value, tick number} pair instead of the row of `out`
  // TICK != 0 - ONE launch per tick (round 5): the streaming front end's side and the model's filterbank (stream_fe.h)
  ww_tick_fe fe;
  ww_fe_filt fb;
};

// Mel-side LDS of the one-launch tick form (stream_fe.h: fe_tick_lds), behind the staged input [WV_T][WV_INLD]; dead before the block loop
#define WT_BASE (WV_T * WV_INLD)  // floats from `lds`; the weights go in in one store round of 12 waves x 16 bytes
#define WT_END (WT_BASE + FE_TL_FLOATS)
static_assert(WT_BASE % 4 == 0, "tick front end: LDS layout");

__device__ __forceinline__ float sigmoid_w(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ void wsync() {
  // LDS traffic of one wave is processed in order; wait for it only (not for outstanding
  // global loads, which an acq_rel fence would also drain) and stop compiler reordering
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// one wave's LDS operations execute in issue order: a scheduling fence is all a wave-private
// write -> read (or read -> overwrite) round trip needs
__device__ __forceinline__ void wsync_fence() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// v_exp_f32 / v_rcp_f32 gates (~1 ulp each, |error| ~2e-7): the gate activations are 16x2 values
// per row and block; with libm tanhf/expf + IEEE division they cost more VALU time than the
// block's MFMAs.
__device__ __forceinline__ float fast_sigmoid_w(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float fast_tanh_w(float x) {
  const float e = __builtin_amdgcn_exp2f(2.8853900817779268f * x);  // exp(2x): inf -> 1, 0 -> -1
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + e);
}

#define MFMA4(acc, av, bv)                                              \
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0); \
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0); \
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0); \
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);

// A block's weights as this lane's MFMA operands: gate [3 taps][sig | tanh], res | skip [3 column tiles]
// (block-uniform base pointers + one 32-bit per-lane offset each: the loads take SGPR base + VGPR offset + immediate, no
//  64-bit address arithmetic on the vector ALU - in the fp32 kernel every vector instruction costs matrix time)
struct wv_wblk { float4 wg[3][2], wrs[3]; };
__device__ __forceinline__ void wv_wload(const wave_args &a, int blk, int j, int kk, wv_wblk &p) {
  const float *wg = a.w_gate4 + (size_t)blk * 3 * 4 * 32 * 4, *wrs = a.w_rs4 + (size_t)blk * 4 * 48 * 4;
  const unsigned og = (unsigned)(kk * 32 + j) * 4, ors = (unsigned)(kk * 48 + j) * 4;
#pragma unroll
  for (int kb = 0; kb < 3; ++kb)
#pragma unroll
    for (int n = 0; n < 2; ++n) p.wg[kb][n] = *(const float4 *)(wg + og + kb * 4 * 32 * 4 + n * 16 * 4);
#pragma unroll
  for (int n = 0; n < 3; ++n) p.wrs[n] = *(const float4 *)(wrs + ors + n * 16 * 4);
}

// the row-major loop's block: the weights and this lane's column of the seven small vectors
struct wave_blk : wv_wblk {
  float bn_s, bn_t, bsig, btanh, bres, bsk0, bsk1;
};
__device__ __forceinline__ void wave_blk_load(const wave_args &a, int blk, int j, int kk, wave_blk &p) {
  wv_wload(a, blk, j, kk, p);
  const float *bn_s = a.bn_s + blk * WV_C, *bn_t = a.bn_t + blk * WV_C, *bg = a.b_gate + blk * 32, *brs = a.b_rs + blk * 48;
  const unsigned uj = (unsigned)j;
  p.bn_s = bn_s[uj];
  p.bn_t = bn_t[uj];
  p.bsig = bg[uj];
  p.btanh = bg[uj + 16];
  p.bres = brs[uj];
  p.bsk0 = brs[uj + 16];
  p.bsk1 = brs[uj + 32];
}


// ---- split-bf16 contractions ("bf16x3") --------------------------------------------------------
// x = hi + lo with hi = bf16(x), lo = bf16(x - hi) carries 16 mantissa bits; a*b is evaluated as
// ah*bh + al*bh + ah*bl by three bf16 MFMAs with fp32 accumulate.  Unlike v_mfma_f32_16x16x4_f32,
// which shares the SIMD's fp32 datapath with the vector ALU (their times add up), the bf16 MFMA
// runs beside it.  Error model and measurements: tools/bf16x3_error.py, DESIGN.md.
//
// The block loop is evaluated TRANSPOSED (channels x time) with v_mfma_f32_16x16x16_bf16: its
// accumulator layout (lane: column n = lane & 15, rows 4*(lane >> 4) + r) has, per lane, exactly
// the four k-values (4*kg .. 4*kg + 3, kg = lane >> 4) its B operand wants for the same column.
// With weights as the A operand (rows = output channels) and activations as B (columns = time),
// the BatchNorm output of a tile IS the undelayed tap's B operand and the gate product IS the
// res/skip conv's B operand - both straight out of registers.  Only the two delayed taps read
// LDS (other time columns, possibly another wave's tile): two 8-byte writes and four 8-byte reads
// per wave and block, one barrier.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// four fp32 values -> (hi, lo) as the 4 x bf16 operand registers
__device__ __forceinline__ void split4(const float (&v)[4], s16x4 &hi, s16x4 &lo) {
  const bf16x2 h01 = __builtin_convertvector((f32x2){v[0], v[1]}, bf16x2);
  const bf16x2 h23 = __builtin_convertvector((f32x2){v[2], v[3]}, bf16x2);
  const unsigned u01 = __builtin_bit_cast(unsigned, h01), u23 = __builtin_bit_cast(unsigned, h23);
  const bf16x2 l01 = __builtin_convertvector((f32x2){v[0] - __uint_as_float(u01 << 16), v[1] - __uint_as_float(u01 & 0xffff0000u)}, bf16x2);
  const bf16x2 l23 = __builtin_convertvector((f32x2){v[2] - __uint_as_float(u23 << 16), v[3] - __uint_as_float(u23 & 0xffff0000u)}, bf16x2);
  const uint2 hv = {u01, u23}, lv = {__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l23)};
  hi = __builtin_bit_cast(s16x4, hv);
  lo = __builtin_bit_cast(s16x4, lv);
}

// v_mfma_f32_16x16x32_bf16 (16 cycles; the K = 16 form costs twice that per MFMA on gfx950, measured):
// its 8 k-slots per lane are filled with TWO such 4-channel groups - k-slots 0..3 of lane group kg
// = channels 4 kg .. 4 kg + 3 of one tap, k-slots 4..7 = the same channels of a second tap (or zeros) -
// which is just a concatenation of two register pairs; the host packs the weights to match.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
struct s16x4_pair { s16x4 lo, hi; };
__device__ __forceinline__ bf16x8 cat8(s16x4 first, s16x4 second) {
  const s16x4_pair p = {first, second};
  return __builtin_bit_cast(bf16x8, p);
}
#define MFMA_BF(acc, av, bv) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// WV_SLOTS A-operand slots per block and its parameter page of WV_PAGE_U4 16-byte units: model_layout.h

// ---- the fp32 transposed block body, the detect head of one 16-row tile and the 16-lane softmax: ONE definition each, used by
//      wavenet_kernel (a window per workgroup) and wavenet_seq_kernel (a sequence walked in chunks, below).  DESIGN.md 4.3: one
//      association of every sum, whatever the dispatch - a time step's chains do not depend on the tile or chunk it sits in.
struct wv_vblk { float4 bns, bnt, bsig, btanh; };
__device__ __forceinline__ f32x4 wv_f4(const float4 &v) { return (f32x4){v.x, v.y, v.z, v.w}; }
// All blocks' small vectors in one LDS table [NB][WV_VT_N][16] (the transposed fp32 loop): ONE definition of its layout.  A lane
// reads its channel group of vector q of block b as the float4 wv_vt(vtab, b, kk)[4 q].
enum { WV_VT_BNS, WV_VT_BNT, WV_VT_BSIG, WV_VT_BTANH, WV_VT_BRES, WV_VT_BSK0, WV_VT_BSK1, WV_VT_N };
#define WV_VT_BLK (WV_VT_N * 16)   // floats per block
#define WV_VT_F (32 * WV_VT_BLK)   // floats of the whole table (NB <= 32)
__device__ __forceinline__ const float4 *wv_vt(const float *vtab, int blk, int kk) { return (const float4 *)(vtab + blk * WV_VT_BLK) + kk; }
// dst_ = entry i_ of the table, fetched from where it lives in the model's arrays (a macro: as a function the address selection
// moved instructions in eight kernels, EXPERIMENTS 14)
#define WV_VT_FETCH(dst_, a_, i_)                                                                                       \
  do {                                                                                                                  \
    const int vb_ = (i_) / WV_VT_BLK, vq_ = ((i_) / 16) % WV_VT_N, vc_ = (i_) & 15;                                      \
    const float *vp_ = vq_ == WV_VT_BNS ? (a_).bn_s + vb_ * WV_C + vc_                                                   \
                       : vq_ == WV_VT_BNT ? (a_).bn_t + vb_ * WV_C + vc_                                                 \
                       : vq_ < WV_VT_BRES ? (a_).b_gate + vb_ * 32 + (vq_ - WV_VT_BSIG) * 16 + vc_                       \
                                          : (a_).b_rs + vb_ * 48 + (vq_ - WV_VT_BRES) * 16 + vc_;                        \
    dst_ = *vp_;                                                                                                        \
  } while (0)
// a block's seven small vectors (this lane's channel group): read from the table one block AHEAD, behind the barrier, so
// that no LDS round trip sits in front of the u write, the accumulators' initial values or the res | skip products
// (the BatchNorm pair and the gate biases, which a block needs at once; the res | skip biases are requested at the top of their
// own block and used ~1,500 cycles later: prefetching all seven costs 56 registers and spills)
__device__ __forceinline__ void wv_vload(const float *vtab, int blk, int kk, wv_vblk &v) {
  const float4 *vt = wv_vt(vtab, blk, kk);
  v.bns = vt[4 * WV_VT_BNS]; v.bnt = vt[4 * WV_VT_BNT]; v.bsig = vt[4 * WV_VT_BSIG]; v.btanh = vt[4 * WV_VT_BTANH];
}
// Written over a wave's MPW tiles (round 5: launches of more than 256 windows run FOUR waves x three tiles, two
// workgroups per CU - the form that gave the split-bf16 loop 14 % at scale; up to 256 windows - one per CU - twelve waves x
// one tile): the tiles' MFMAs and gate evaluations are independent instructions back to back, the per-tile arithmetic is
// the same source in both forms, so a posterior does not depend on the launch size.
// UPL: floats per channel-group plane of a u buffer ((rows + WV_PAD) * 4); tl: this lane's time column in the wave's first tile.
// HIST (the sequence form): the WV_PAD rows in front of u are not zeros but the block's last WV_PAD rows of u from the chunk
// before - hist[blk][kk][row][4], parked in the pad rows in front of the barrier by the wave with hist_wave set, and replaced
// behind it by rows [valid, valid + WV_PAD) of [pad | u], i.e. the last WV_PAD rows up to the chunk's last valid row.  One
// wave does both and a wave's LDS operations complete in issue order, so the history needs no barrier of its own.
// (DIL - where a SET kernel, whose `a` is a moved COPY of its arguments, reads the dilations: an index into a local copy would keep
//  it in scratch memory.  0: a.dil4[blk / 16], the arguments themselves.  1 - wavenet_seq_kernel<SET>, which has moved its arguments
//  in place and has only the copy: the word is picked by a comparison.  2 - wavenet_kernel<SET>: from geo, the kernel's arguments as
//  they came; with the comparison its one-launch tick forms held every argument in scalar registers from the top, 106 of them, and
//  spilled four)
template <int MPW, int UPL, bool HIST, int DIL = 0>
__device__ __forceinline__ void wv_block_t(const wave_args &a, int blk, float *ubuf, const float *vtab, int j, int kk, int tl,
                                           f32x4 (&x)[MPW], f32x4 (&skip)[MPW][2], const wv_wblk &P, wv_wblk &Pnext,
                                           const wv_vblk &V, wv_vblk &Vnext, float *hist = nullptr, int valid = 0,
                                           bool hist_wave = false, const wave_args *geo = nullptr) {
  float *u = ubuf + (blk & 1) * 4 * UPL + kk * UPL + WV_PAD * 4;          // row 0 of this lane's channel-group plane
  int d;
  if constexpr (DIL == 1) d = (int)(((blk < 16 ? a.dil4[0] : a.dil4[1]) >> (4 * (blk & 15))) & 15);
  else if constexpr (DIL == 2) d = (int)((geo->dil4[blk >> 4] >> (4 * (blk & 15))) & 15);
  else d = (int)((a.dil4[blk >> 4] >> (4 * (blk & 15))) & 15);
  const float4 *vt = wv_vt(vtab, blk, kk);
  const float4 bres = vt[4 * WV_VT_BRES], bsk0 = vt[4 * WV_VT_BSK0], bsk1 = vt[4 * WV_VT_BSK1];
  f32x4 uv[MPW], as[MPW], at[MPW];
  f32x4 hv = {0.f, 0.f, 0.f, 0.f};
  if (HIST && hist_wave) hv = *(const f32x4 *)(hist + blk * (4 * WV_PAD * 4) + (kk * WV_PAD + j) * 4);
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi) {
    uv[mi] = (f32x4){x[mi][0] * V.bns.x + V.bnt.x, x[mi][1] * V.bns.y + V.bnt.y, x[mi][2] * V.bns.z + V.bnt.z,
                     x[mi][3] * V.bns.w + V.bnt.w};
    *(f32x4 *)(u + (tl + 16 * mi) * 4) = uv[mi];
  }
  const int nb = blk + 1 < a.NB ? blk + 1 : blk;
  wv_wload(a, nb, j, kk, Pnext);  // unconditional (clamped) prefetch, as the row-major loop
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi) {
    as[mi] = wv_f4(V.bsig);
    at[mi] = wv_f4(V.btanh);
    MFMA4(as[mi], P.wg[2][0], uv[mi]);             // tap 2 = this row: runs while the other waves arrive
    MFMA4(at[mi], P.wg[2][1], uv[mi]);
  }
  if (HIST && hist_wave) *(f32x4 *)(u + (j - WV_PAD) * 4) = hv;
  __syncthreads();  // u complete (all rows, all waves)
  f32x4 t0v[MPW], t1v[MPW];
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi) {            // rows < 0 hit the pad (d <= 8)
    t0v[mi] = *(const f32x4 *)(u + (tl + 16 * mi - 2 * d) * 4);
    t1v[mi] = *(const f32x4 *)(u + (tl + 16 * mi - d) * 4);
  }
  wv_vload(vtab, nb, kk, Vnext);
  if (HIST && hist_wave) hv = *(const f32x4 *)(u + (valid - WV_PAD + j) * 4);
  __builtin_amdgcn_sched_barrier(0);  // the tap reads (and the table reads behind them) are in flight before the first wait
  const int has_res = (a.has_res_mask >> blk) & 1;
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi) {
    MFMA4(as[mi], P.wg[0][0], t0v[mi]);
    MFMA4(at[mi], P.wg[0][1], t0v[mi]);
    MFMA4(as[mi], P.wg[1][0], t1v[mi]);
    MFMA4(at[mi], P.wg[1][1], t1v[mi]);
  }
  if (HIST && hist_wave) *(f32x4 *)(hist + blk * (4 * WV_PAD * 4) + (kk * WV_PAD + j) * 4) = hv;
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi) {
    const f32x4 gv = {fast_tanh_w(at[mi][0]) * fast_sigmoid_w(as[mi][0]), fast_tanh_w(at[mi][1]) * fast_sigmoid_w(as[mi][1]),
                      fast_tanh_w(at[mi][2]) * fast_sigmoid_w(as[mi][2]), fast_tanh_w(at[mi][3]) * fast_sigmoid_w(as[mi][3])};
    f32x4 ar = wv_f4(bres), s0 = wv_f4(bsk0), s1 = wv_f4(bsk1);
    // (hand-interleaving the k-steps of the accumulators - dependent MFMAs issue after 40 cycles, independent ones after 32 - was
    //  1 % SLOWER: with three waves per SIMD the other waves fill those 8 cycles, and the compiler's own order keeps fewer values live)
    if (has_res) { MFMA4(ar, P.wrs[0], gv); }
    MFMA4(s0, P.wrs[1], gv);
    MFMA4(s1, P.wrs[2], gv);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (has_res) x[mi][r] = relu1(ar[r]) + x[mi][r];
      skip[mi][0][r] = skip[mi][0][r] + relu1(s0[r]);
      skip[mi][1][r] = skip[mi][1][r] + relu1(s1[r]);
    }
  }
}

// The detect head's two 1x1 convs on one 16-row tile: ReLU(skip sums) -> 32 -> ReLU -> NOUT (padded to 16), through the wave-private
// tile ht [16][32].  Returns the logits WITHOUT the last bias: register r of a lane = row 4 kk + r of the tile, column j.
struct wv_head_w { float4 w1[2][2], w2[2]; float b1a, b1b, b2; };
__device__ __forceinline__ void wv_head_load(const wave_args &a, int j, int kk, wv_head_w &h) {
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
    for (int n = 0; n < 2; ++n) h.w1[kb][n] = *(const float4 *)(a.d_w1_4 + (unsigned)((kb * 4 + kk) * 32 + n * 16 + j) * 4);
    h.w2[kb] = *(const float4 *)(a.d_w2_4 + (unsigned)((kb * 4 + kk) * 16 + j) * 4);
  }
  const unsigned uj = (unsigned)j;  // (uniform base + one 32-bit per-lane offset, as wave_blk_load)
  h.b1a = a.d_b1[uj]; h.b1b = a.d_b1[uj + 16]; h.b2 = a.d_b2[uj];
}
template <bool TRANSPOSED>
__device__ __forceinline__ f32x4 wv_head_tile(const f32x4 (&sk)[2], float *ht, const wv_head_w &h, int j, int kk) {
  if (TRANSPOSED) {
    *(float4 *)(ht + j * WV_S + kk * 4) = make_float4(fmaxf(sk[0][0], 0.f), fmaxf(sk[0][1], 0.f), fmaxf(sk[0][2], 0.f), fmaxf(sk[0][3], 0.f));
    *(float4 *)(ht + j * WV_S + 16 + kk * 4) = make_float4(fmaxf(sk[1][0], 0.f), fmaxf(sk[1][1], 0.f), fmaxf(sk[1][2], 0.f), fmaxf(sk[1][3], 0.f));
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ht[(kk * 4 + r) * WV_S + j] = fmaxf(sk[0][r], 0.f);
      ht[(kk * 4 + r) * WV_S + 16 + j] = fmaxf(sk[1][r], 0.f);
    }
  }
  wsync();
  f32x4 h0 = {0.f, 0.f, 0.f, 0.f}, h1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    const float4 av = *(const float4 *)(ht + j * WV_S + kb * 16 + kk * 4);
    MFMA4(h0, av, h.w1[kb][0]);
    MFMA4(h1, av, h.w1[kb][1]);
  }
  wsync();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    ht[(kk * 4 + r) * WV_S + j] = fmaxf(h0[r] + h.b1a, 0.f);
    ht[(kk * 4 + r) * WV_S + 16 + j] = fmaxf(h1[r] + h.b1b, 0.f);
  }
  wsync();
  f32x4 y = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    const float4 av = *(const float4 *)(ht + j * WV_S + kb * 16 + kk * 4);
    MFMA4(y, av, h.w2[kb]);
  }
  wsync();
  return y;
}

// softmax over the NOUT <= 16 pooled logits held by lanes 0..15 of a wave (lane c = column c; call it from those lanes): the
// value of this lane's column
__device__ __forceinline__ float wv_softmax16(float v, int c, int NOUT) {
  float mx = (c < NOUT) ? v : -INFINITY;
  for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float e = (c < NOUT) ? expf(v - mx) : 0.f;
  float sum = e;
  for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o);
  return e / sum;
}

// LDS of wavenet_kernel, in floats (NB <= 32): ONE set of offsets; the kernel's array is sized from them.
//   fp32:       [ u[2][WV_T + WV_PAD][16] | g [WV_T][16], later the head tile [WV_T][32] ] | vector table (transposed loop only)
//   split-bf16: [ u planes (the fp32 u buffers' bytes) | three parameter pages (the head tile over them) | BatchNorm table ]
//   under both, in the prologue only: the staged input [WV_T][WV_INLD] and, one-launch tick, the front end's mel side behind it
constexpr int WV_U_F = 2 * (WV_T + WV_PAD) * WV_C;  // the two u buffers, causal pad rows included
constexpr int WV_H_F = WV_T * WV_S;                 // the head tile (its first half: the row-major loop's g tiles)
constexpr int WV_IN_F = WV_T * WV_INLD;             // the staged input
constexpr int WV_PG_F = 3 * WV_PAGE_U4 * 4;         // three parameter pages
constexpr int WV_BN_F = 32 * 8 * 4;                 // BatchNorm table [NB][2][4] float4
static_assert(WV_H_F <= WV_PG_F, "the head tile lies over the parameter pages");
#define WV_NVT(threads_) ((WV_VT_F + (threads_) - 1) / (threads_))        // vector-table entries per thread
#define WV_NPL(threads_) ((WV_PAGE_U4 + (threads_) - 1) / (threads_))    // pieces of a parameter page per thread (the last one partial)

// All NB blocks through wv_block_t<MPW_, UPL_, HIST_>: the parameters one block ahead in two register sets, the loop unrolled by
// two.  pw_[0]: block 0's weights, requested in front of the barrier that publishes the vector table; the trailing arguments are
// wv_block_t's hist, valid, hist_wave; SET is the kernel's template parameter.  (A macro: as a function template the twelve-wave sequence kernels spilled 12 bytes,
// EXPERIMENTS 14.)
#define WV_BLOCKS_T(MPW_, UPL_, HIST_, DIL_, a_, ubuf_, vtab_, j_, kk_, tl_, x_, skip_, pw_, ...)                                        \
  do {                                                                                                                             \
    wv_vblk pv[2];                                                                                                                 \
    wv_vload(vtab_, 0, kk_, pv[0]);                                                                                                \
    for (int blk = 0; blk < (a_).NB; blk += 2) {                                                                                   \
      wv_block_t<MPW_, UPL_, HIST_, DIL_>(a_, blk, ubuf_, vtab_, j_, kk_, tl_, x_, skip_, pw_[0], pw_[1], pv[0], pv[1], ##__VA_ARGS__);  \
      if (blk + 1 < (a_).NB)                                                                                                       \
        wv_block_t<MPW_, UPL_, HIST_, DIL_>(a_, blk + 1, ubuf_, vtab_, j_, kk_, tl_, x_, skip_, pw_[1], pw_[0], pv[1], pv[0], ##__VA_ARGS__); \
    }                                                                                                                              \
  } while (0)

// Where a posterior goes (lane c_ holds column c_ of launch row w_ + k_): a streaming tick's as ONE 8-byte {value, tick number} store
// the host polls (common.h), anything else as its row of `out`.  (A macro: as a function it moved instructions in the four fp32
// one-launch tick kernels, EXPERIMENTS 14.)
#define WV_POST_STORE(tag_, out_, NOUT_, w_, k_, c_, p_)                       \
  do {                                                                        \
    if ((tag_).slots) {                                                       \
      if ((c_) == (tag_).pidx) tick_tag_store(tag_, w_, p_, k_);              \
    } else if ((c_) < (NOUT_)) {                                              \
      (out_)[(size_t)((w_) + (k_)) * (NOUT_) + (c_)] = (p_);                  \
    }                                                                         \
  } while (0)

// Input 1x1 conv + ReLU of one 16-row tile of the staged input -> x_ in accumulator layout, and the tile's skip sums start at zero.
// row_: this lane's row j of the tile, in rows of in_lds_.  TR_: the operands swapped - lane = time column, registers = channels
// 4 kk + r, bias b_in_[4 kk + r]; otherwise lane = column j (bias_: its b_in), registers = rows 4 kk + r.  (A macro: as a function
// template it moved instructions in eight window and sequence kernels, EXPERIMENTS 14.)
#define WV_INPUT_TILE(TR_, in_lds_, row_, kk_, bw_, b_in_, bias_, x_, skip_)                          \
  do {                                                                                                \
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};                                                                 \
    _Pragma("unroll") for (int kb = 0; kb < 3; ++kb) {                                                \
      const float4 av = *(const float4 *)((in_lds_) + (row_) * WV_INLD + kb * 16 + (kk_) * 4);        \
      if (TR_) {                                                                                      \
        MFMA4(acc, bw_[kb], av);                                                                      \
      } else {                                                                                        \
        MFMA4(acc, av, bw_[kb]);                                                                      \
      }                                                                                               \
    }                                                                                                 \
    _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                     \
      x_[r] = fmaxf(acc[r] + ((TR_) ? (b_in_)[(unsigned)((kk_) * 4 + r)] : (bias_)), 0.f);            \
    skip_[0] = (f32x4){0.f, 0.f, 0.f, 0.f};                                                           \
    skip_[1] = (f32x4){0.f, 0.f, 0.f, 0.f};                                                           \
  } while (0)

// a time step's skip sum (the encoder's output row e [32]) out of the transposed state: lane = time column, four consecutive
// channels per register quad
__device__ __forceinline__ void wv_enc_store_t(float *e, int kk, const f32x4 (&sk)[2]) {
  *(float4 *)(e + kk * 4) = make_float4(sk[0][0], sk[0][1], sk[0][2], sk[0][3]);
  *(float4 *)(e + 16 + kk * 4) = make_float4(sk[1][0], sk[1][1], sk[1][2], sk[1][3]);
}

// Staging a window of wavenet_kernel, in_lds[t][0..47] = the window's n4_ float4s (a contiguous [rows][n_mel] block, n_mel % 4 == 0,
// 16-byte aligned) and zeros elsewhere, in three steps.  All of a thread's 16-byte loads are issued first (unconditional, from clamped
// addresses: nothing for the next load to wait for), the zero fill runs while they are in flight, then - behind a barrier - the
// 16-byte LDS stores.  tid_ / threads_: the thread and the workgroup's size.  (Macros: as functions over a small struct they moved
// instructions in all eleven window kernels, EXPERIMENTS 14.)
#define WV_STAGE_SQ(threads_) ((WV_T * WV_INLD / 4 + (threads_) - 1) / (threads_))  // float4s per thread
#define WV_STAGE_REQUEST(st_, src_, n4_, tid_, threads_)                          \
  do {                                                                            \
    _Pragma("unroll") for (int sq_ = 0; sq_ < WV_STAGE_SQ(threads_); ++sq_) {     \
      const int si_ = (tid_) + sq_ * (threads_);                                  \
      st_[sq_] = *(const f32x4 *)((src_) + 4 * (si_ < (n4_) ? si_ : (n4_) - 1));  \
    }                                                                             \
  } while (0)
#define WV_STAGE_ZERO(in_lds_, tid_, threads_)                                    \
  do {                                                                            \
    for (int si_ = (tid_); si_ < WV_T * WV_INLD / 4; si_ += (threads_))           \
      ((float4 *)(in_lds_))[si_] = make_float4(0.f, 0.f, 0.f, 0.f);               \
  } while (0)
#define WV_STAGE_STORE(st_, in_lds_, n4_, n_mel_, tid_, threads_)                 \
  do {                                                                            \
    _Pragma("unroll") for (int sq_ = 0; sq_ < WV_STAGE_SQ(threads_); ++sq_) {     \
      const int si_ = (tid_) + sq_ * (threads_);                                  \
      if (si_ < (n4_)) {                                                          \
        const int se_ = si_ * 4, st0_ = se_ / (n_mel_), sc_ = se_ - st0_ * (n_mel_); \
        *(f32x4 *)((in_lds_) + st0_ * WV_INLD + sc_) = st_[sq_];                  \
      }                                                                           \
    }                                                                             \
  } while (0)

// FP32T: the fp32 block loop in the TRANSPOSED form of the split-bf16 loop (channels x time; round 3) - see its comment below.
// TICK = 1 / 2 (fp32 / fp64 transform) - ONE launch per streaming tick (round 5; crnn.hip's crnn_stream_kernel<FE> has the full
// story): workgroup 2 s + k is window k of stream s's tick; it reads the stream's control words and samples over the bus, waves
// 0 and 1 transform the new frames (one each) straight into the staged input while the others stage the rows that were
// there before; the workgroup of the tick's newest window alone writes the stream's state (mel rows, sample ring and carry -
// the latter two ping-pong by the stream's parity, so its sibling still reads last tick's).  Twelve waves x one tile only.
// SET (a model set: ww_set_forward_windows_dev, or a bank created from one): the workgroup's member is set.ids[i] - a batch: its
// window; a one-launch tick: its stream, blockIdx.x / 2; a two-launch tick: the stream in its window's aux word (stream *
// WW_STREAM_GXC + ...) -, and the weight pointers move on to that member's block before anything is read through them.  fp32
// transposed forms only.
// (three parts.  wavenet_kernel leaves its arguments where they are and reads the weights of each phase through a copy made where
//  the phase begins, WV_SET_VIEW; wavenet_seq_kernel moves all of them at its top)
__device__ __forceinline__ void wv_set_move_front(wave_args &a, long long off) {  // the input conv and the per-block vectors
  ww_set_move(a.w_in4, off); ww_set_move(a.b_in, off); ww_set_move(a.bn_s, off); ww_set_move(a.bn_t, off);
  ww_set_move(a.b_gate, off); ww_set_move(a.b_rs, off); ww_set_move(a.wpk, off);
}
__device__ __forceinline__ void wv_set_move_blocks(wave_args &a, long long off) {
  ww_set_move(a.w_gate4, off); ww_set_move(a.w_rs4, off);
}
__device__ __forceinline__ void wv_set_move_head(wave_args &a, long long off) {
  ww_set_move(a.d_w1_4, off); ww_set_move(a.d_b1, off); ww_set_move(a.d_w2_4, off); ww_set_move(a.d_b2, off);
}
// name_: `a` itself (SET = false), or a copy of it - the whole struct, so that a field added later cannot be missing from it - whose
// pointers mover_ has moved on by set_off.  The copy is made where the phase that reads it begins (the empty asm makes the moved
// pointers values of THAT place: formed at the top they were held from there), and nothing indexes into it: the dilations, the one
// array of wave_args, are read from `a` itself (wv_block_t's DIL = 2) - an index into a local copy would keep it in scratch memory.
#define WV_SET_VIEW(name_, mover_)                                          \
  wave_args name_##_m;                                                      \
  if constexpr (SET) {                                                      \
    name_##_m = a;                                                          \
    long long off_ = set_off;                                               \
    asm volatile("" : "+s"(off_));                                          \
    mover_(name_##_m, off_);                                                \
  }                                                                         \
  const wave_args &name_ = SET ? name_##_m : a;
template <bool HEAD_ONLY, bool SPLIT_BF16, int WV_NW, bool FP32T = false, int TICK = 0, bool SET = false>
__global__ __launch_bounds__(WV_NW * 64, WV_NW == 12 ? (SPLIT_BF16 ? WV_BF16_OCC : 3) : 2) void wavenet_kernel(wave_args a, ww_set_ref set) {
  static_assert(!SET || (FP32T && !HEAD_ONLY), "model sets run the fp32 transposed forms");
  [[maybe_unused]] long long set_off = 0;
  if constexpr (SET) {
    const int wg = blockIdx.x;
    set_off = ww_set_offset(set, TICK ? wg >> 1 : set.aux ? set.aux[wg] / WW_STREAM_GXC : wg);
  }
  constexpr int WV_MPW = 12 / WV_NW, WV_THREADS = WV_NW * 64;
  static_assert(!TICK || (WV_NW == 12 && !HEAD_ONLY), "the one-launch tick runs twelve waves x one tile");
  constexpr bool TRANSPOSED = SPLIT_BF16 || FP32T;  // state layout: lane = time column, four consecutive channels per register quad
  static_assert(!(SPLIT_BF16 && FP32T), "one arithmetic mode");
  static_assert(WV_MPW * WV_NW == 12, "12 row tiles");
  constexpr int BLOCKS_F = SPLIT_BF16 ? WV_U_F + WV_PG_F + WV_BN_F : FP32T ? WV_U_F + WV_H_F + WV_VT_F : WV_U_F + WV_H_F;
  constexpr int STAGE_F = TICK ? WT_END : WV_IN_F;
  __shared__ __align__(16) float lds[BLOCKS_F > STAGE_F ? BLOCKS_F : STAGE_F];
  __shared__ float red[WV_NW][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kk = lane >> 4;
  const int w = blockIdx.x;
  const int T = a.T;

  f32x4 x[WV_MPW], skip[WV_MPW][2];
  float *ubuf = lds;                                    // [2][WV_T + WV_PAD][16]
  float *gbuf = lds + WV_U_F;                             // [WV_T][16] (wave-private tiles)
  float *hbuf = gbuf;                                   // detect head reuses it as [WV_T][32]
  if (HEAD_ONLY) {
    // detect.tflite alone (reference detect_model(x), wakeword/tflite.py:231): skip sums come from memory
    const float *e = a.enc_in + (size_t)w * T * WV_S;
#pragma unroll
    for (int mi = 0; mi < WV_MPW; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = (wave * WV_MPW + mi) * 16 + kk * 4 + r;
        skip[mi][0][r] = t < T ? e[(size_t)t * WV_S + j] : 0.f;
        skip[mi][1][r] = t < T ? e[(size_t)t * WV_S + 16 + j] : 0.f;
      }
    (void)x; (void)ubuf;
  } else {
  int64_t row = 0;
  int valid = 0;
  // ---- TICK: over the bus, together: the tick's 320 samples (40 x 16 bytes) and the stream's control words
  typedef typename std::conditional<TICK == 2, double, float>::type RT;
  uint4 t_raw = make_uint4(0u, 0u, 0u, 0u);
  int4 t_cw = make_int4(0, 0, 0, 0);
  if (TICK) {
    if (tid < 40) t_raw = ((const uint4 *)(a.fe.frames + (size_t)(w >> 1) * WW_CHUNK))[tid];
    t_cw = ((const int4 *)a.fe.ctl)[w >> 1];
  } else if (a.wa.row && a.wa.valid) {  // (both tables: the two loads go out together)
    const int64_t r_ = a.wa.row[w];
    const int v_ = a.wa.valid[w];
    row = r_;
    valid = v_;
  } else {  // (plain ifs: as `p ? p[w] : constant` the compiler parked the constant in scratch memory to select between two addresses)
    row = a.wa.row0 + (int64_t)w * a.wa.hop;
    valid = a.wa.valid_const;
    if (a.wa.row) row = a.wa.row[w];
    if (a.wa.valid) valid = a.wa.valid[w];
  }
  if (!TICK) {
    if (valid > T) valid = T;
    if (row + valid > a.wa.mel_rows) valid = (int)(a.wa.mel_rows - row);
    if (valid < 0) valid = 0;
  }

  // the input conv's operands: requested now, used behind the staging
  WV_SET_VIEW(af, wv_set_move_front)
  float4 bw[3];
#pragma unroll
  for (int kb = 0; kb < 3; ++kb) bw[kb] = *(const float4 *)(af.w_in4 + ((size_t)(kb * 4 + kk) * 16 + j) * 4);
  const float bias = af.b_in[j];
  // ... and what the block loop's LDS tables are filled from (split-bf16: parameter pages 0 and 1 and the BatchNorm table; fp32
  // transposed: the per-block vector table): requested here, parked in LDS once the staged input is dead - as loops of
  // "load, store" behind the input conv they were three to four round trips to L2 in a row on every window's critical path
  constexpr int NPL = WV_NPL(WV_THREADS);
  static_assert(NPL >= 2 && NPL <= 4, "page pieces per thread");
  constexpr int NVT = WV_NVT(WV_THREADS);
  // (clang ext-vector elements: arrays of HIP's struct vector types stayed in scratch memory)
  u32x4 pg0[NPL], pg1[NPL];
  f32x4 bnv = {0.f, 0.f, 0.f, 0.f};
  float vte[NVT];
  if (SPLIT_BF16) {
    const int second = a.NB > 1 ? 1 : 0;
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
      const int i = tid + q * WV_THREADS < WV_PAGE_U4 ? tid + q * WV_THREADS : WV_PAGE_U4 - 1;
      pg0[q] = *(const u32x4 *)(a.wpk + i);
      pg1[q] = *(const u32x4 *)(a.wpk + (size_t)second * WV_PAGE_U4 + i);
    }
    const int bi = tid < a.NB * 8 ? tid : 0;                                    // [NB][2][4] float4 = scale, shift (NB <= 32 <= threads / 8)
    bnv = *(const f32x4 *)(((bi >> 2) & 1 ? a.bn_t : a.bn_s) + (bi >> 3) * WV_C + 4 * (bi & 3));
  }
  if (FP32T) {
#pragma unroll
    for (int q = 0; q < NVT; ++q) {
      int i = tid + q * WV_THREADS;
      i = i < a.NB * WV_VT_BLK ? i : 0;
      WV_VT_FETCH(vte[q], af, i);
    }
  }

  // ---- stage the window: in_lds[t][0..47], zero outside [0,valid) x [0,n_mel)
  float *in_lds = lds;
  if constexpr (TICK != 0) {
    const ww_tick_fe &fe = a.fe;
    const int s = w >> 1, k = w & 1;
    // device-side inputs of the front end that do not depend on the control words: requested while those cross the bus
    const f32x4 wlq = ((const f32x4 *)a.fb.wpad)[tid < WW_MEL_TAPS * 64 / 4 ? tid : 0];
    const int mel_st = lane < a.n_mel ? a.fb.start[lane] : 0;
    const float mel_bias = lane < a.n_mel ? a.fb.bias[lane] : 0.0f;
    // the sample ring: threads 0..127 ask for the copy of parity 0, threads 128..255 for parity 1 (128 x 4 = 512 > fill)
    const f32x4 ringq = ((const f32x4 *)(fe.ring + ((size_t)((tid >> 7) & 1) * fe.S + s) * WW_ST_RING))[tid & 127];
    const float carry0 = fe.prev[s], carry1 = fe.prev[fe.S + s];
    fft_consts<RT> fc;
    if (wave < 2) fft_load_consts<RT>(fc, lane, a.fb.hann, a.fb.tw256, a.fb.tw512);
    // ---- what this workgroup is (uniform over it)
    const int slots = T + 1;
    const fe_tick_ctl c = fe_tick_decode(t_cw, k, slots);
    if (c.idle) return;
    // the rows that were there before: the block [(pos + k + 2) % (T + 1), + T - nfk) of the stream's mirrored ring
    f32x4 st[WV_STAGE_SQ(WV_THREADS)];
    int n4 = 0;
    if (c.window) {
      const float *src = a.mel + ((size_t)s * fe.HR + c.b) * a.n_mel;  // (160-byte rows of a hipMalloc'ed history: 16-byte aligned)
      n4 = ((T - c.nfk) * a.n_mel) >> 2;
      WV_STAGE_REQUEST(st, src, n4, tid, WV_THREADS);
    }
    const fe_tick_lds<RT> l = FE_TICK_LDS(RT, lds + WT_BASE);
    ((f32x4 *)l.wl)[tid] = wlq;
    if (tid < 256 && (tid >> 7) == c.par) ((f32x4 *)l.x)[tid & 127] = ringq;
    if (tid < 40) ((uint4 *)l.xs)[tid] = t_raw;
    if (c.window) WV_STAGE_ZERO(in_lds, tid, WV_THREADS);
    __syncthreads();
    // ---- [ring | new samples]: normalise, clip, pre-emphasise
    for (int i = tid; i < WW_CHUNK; i += WV_THREADS) l.x[c.fill + i] = fe_sample(l.xs, i, c.par ? carry1 : carry0, fe.cv);
    if (c.window) WV_STAGE_STORE(st, in_lds, n4, a.n_mel, tid, WV_THREADS);  // (the zero fill is complete: the old rows go in beside the normalisation)
    __syncthreads();
    // tflite.py:156-158: the carry is the un-emphasised last sample
    if (c.writer && tid == 0) fe.prev[(size_t)(c.par ^ 1) * fe.S + s] = fe_norm(l.xs[WW_CHUNK - 1], fe.cv);
    // ---- new frames: wave f transforms frame f; its mel row goes straight into the staged input (row T - nfk + f) and, from
    // the writer, into the stream's mirrored ring
    if (wave < c.nfk) {
      const float mv = fe_frame_mel<RT>(l.x + wave * fe.hop, fc, l.buf, l.mag, wave, l.wl, mel_st, mel_bias, a.fb, lane);
      if (lane < a.n_mel) {
        in_lds[(T - c.nfk + wave) * WV_INLD + lane] = mv;
        if (c.writer) fe_ring_store(fe.hist, (size_t)s * fe.HR, c.pos + wave, slots, a.n_mel, lane, mv);
      }
    }
    if (c.writer) {  // keep the ring tail (for the next tick: the other copy)
      const int keep = c.fill + WW_CHUNK - c.nf * fe.hop;
      float *ring = fe.ring + ((size_t)(c.par ^ 1) * fe.S + s) * WW_ST_RING;
      for (int i = tid; i < keep; i += WV_THREADS) ring[i] = l.x[c.nf * fe.hop + i];
    }
    if (!c.window) return;  // the tick has no window for this stream: its ring has advanced, that is all
  } else {
    const float *src = a.mel + row * a.n_mel;
    const int n = valid * a.n_mel;
    if ((a.n_mel & 3) == 0 && ((((uintptr_t)src) & 15) == 0)) {
      // the window is one contiguous [valid][n_mel] block and a row is a whole number of float4s
      const int n4 = n >> 2;
      f32x4 st[WV_STAGE_SQ(WV_THREADS)];
#pragma unroll
      for (int q = 0; q < WV_STAGE_SQ(WV_THREADS); ++q) st[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (n4 > 0) WV_STAGE_REQUEST(st, src, n4, tid, WV_THREADS);
      WV_STAGE_ZERO(in_lds, tid, WV_THREADS);
      __syncthreads();
      WV_STAGE_STORE(st, in_lds, n4, a.n_mel, tid, WV_THREADS);
    } else {  // any other pointer or row length: four bytes at a time
      WV_STAGE_ZERO(in_lds, tid, WV_THREADS);
      __syncthreads();
      for (int i = tid; i < n; i += WV_THREADS) {
        int t = i / a.n_mel, c = i - t * a.n_mel;
        in_lds[t * WV_INLD + c] = src[i];
      }
    }
  }
  __syncthreads();

  // ---- input 1x1 conv + ReLU -> x in accumulator layout.  m-tile mi of this wave covers rows
  // (wave*3 + mi)*16 .. +15; lane holds rows kk*4 + r, column j.
#pragma unroll
  for (int mi = 0; mi < WV_MPW; ++mi) WV_INPUT_TILE(TRANSPOSED, in_lds, (wave * WV_MPW + mi) * 16 + j, kk, bw, af.b_in, bias, x[mi], skip[mi]);
  __syncthreads();  // in_lds is dead from here on

  if (FP32T) {
    // ---- fp32 block loop, transposed (lane = time column t0 + j, registers = channels 4 kk + r), on v_mfma_f32_16x16x4_f32 with
    //      the weights as the A operand.  The packed weights of the row-major loop serve as they are: k-step q of lane group
    //      kk is input channel 4 kk + q in both forms.  What the transposition buys (as in the split-bf16 loop): the BatchNorm
    //      output of a tile IS the undelayed tap's B operand and the gate product IS the res | skip conv's B operand - both
    //      straight from registers.  LDS per block and wave: ONE 16-byte write (u, for the delayed taps of other rows) and
    //      TWO 16-byte reads (rows t - 2d, t - d), against 8 four-byte writes, 4 sixteen-byte reads and two wave-private
    //      round trips (u -> A operand, gate product -> A operand) in the row-major loop.  u is stored channel-group-major,
    //      [kk][row][4 floats] with the four planes a multiple of 256 bytes apart: consecutive lanes of a group touch
    //      consecutive 16 bytes and the lane groups of ds_read_b128 / ds_write_b128 (MI355X_MICROARCH.md, LDS) cover all 64 banks
    //      once (row-major [row][16] put the 8 lanes of a write group on 2 bank quads: 5.3 M conflict cycles per 256 windows).  The conv biases are the
    //      accumulators' initial values (per-lane float4 by channel group); all blocks' small vectors sit in one LDS table.
    float *vtab = hbuf + WV_H_F;
#pragma unroll
    for (int q = 0; q < NVT; ++q) {
      const int i = tid + q * WV_THREADS;
      if (i < a.NB * WV_VT_BLK) vtab[i] = vte[q];
    }
    constexpr int UPL = (WV_T + WV_PAD) * 4;  // floats per channel-group plane
    static_assert(UPL % 64 == 0, "u planes must start on the same bank");
    for (int i = tid; i < 2 * 4 * WV_PAD * 4; i += WV_THREADS) {  // causal zero rows of both u buffers, every plane
      const int b = i / (4 * WV_PAD * 4), k = (i / (WV_PAD * 4)) & 3, o = i % (WV_PAD * 4);
      ubuf[b * 4 * UPL + k * UPL + o] = 0.f;
    }
    wv_wblk pw[2];
    WV_SET_VIEW(ab, wv_set_move_blocks)
    wv_wload(ab, 0, j, kk, pw[0]);
    const int tl = wave * WV_MPW * 16 + j;  // this lane's time column in the wave's first tile (tile mi: + 16 mi)
    __syncthreads();               // table + zero rows
    if constexpr (SET) WV_BLOCKS_T(WV_MPW, UPL, false, 2, ab, ubuf, vtab, j, kk, tl, x, skip, pw, (float *)nullptr, 0, false, &a);
    else WV_BLOCKS_T(WV_MPW, UPL, false, 0, a, ubuf, vtab, j, kk, tl, x, skip, pw);
    __syncthreads();
  } else if (!SPLIT_BF16) {
  // causal zero rows of both u buffers
  for (int i = tid; i < 2 * WV_PAD * WV_C; i += WV_THREADS) {
    int b = i / (WV_PAD * WV_C), o = i - b * (WV_PAD * WV_C);
    ubuf[b * (WV_T + WV_PAD) * WV_C + o] = 0.f;
  }

  // block parameters are prefetched one block ahead (two register sets, loop unrolled by two)
  wave_blk pb[2];
  wave_blk_load(a, 0, j, kk, pb[0]);
  auto run_block = [&](int blk, const wave_blk &P, wave_blk &Pnext) {
    float *u = ubuf + (blk & 1) * (WV_T + WV_PAD) * WV_C + WV_PAD * WV_C;  // row 0 of u
    const int d = (int)((a.dil4[blk >> 4] >> (4 * (blk & 15))) & 15);  // kernel-argument SGPRs, no load
    // ---- BatchNorm affine (wavenet_model.py:57) -> LDS
#pragma unroll
    for (int mi = 0; mi < WV_MPW; ++mi) {
      const int t0 = (wave * WV_MPW + mi) * 16 + kk * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) u[(t0 + r) * WV_C + j] = x[mi][r] * P.bn_s + P.bn_t;
    }
    // next block's parameters: issued unconditionally (index clamped) - a conditional prefetch makes
    // the compiler drain ALL outstanding loads at the join, i.e. wait for the prefetch it just issued
    wave_blk_load(a, blk + 1 < a.NB ? blk + 1 : blk, j, kk, Pnext);
    const float bsig = P.bsig, btanh = P.btanh, bres = P.bres, bsk0 = P.bsk0, bsk1 = P.bsk1;
    const int has_res = (a.has_res_mask >> blk) & 1;
    __syncthreads();  // u complete (all rows, all waves)

#pragma unroll
    for (int mi = 0; mi < WV_MPW; ++mi) {
      const int t0 = (wave * WV_MPW + mi) * 16;
      f32x4 as = {0.f, 0.f, 0.f, 0.f}, at = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < 3; ++kb) {
        // tap kb reads u[t - (2 - kb) * d]; rows < 0 hit the zero pad (d <= 8 -> >= -16)
        const float4 av = *(const float4 *)(u + (t0 + j - (2 - kb) * d) * WV_C + kk * 4);
        MFMA4(as, av, P.wg[kb][0]);
        MFMA4(at, av, P.wg[kb][1]);
      }
      float *gt = gbuf + t0 * WV_C;
#pragma unroll
      for (int r = 0; r < 4; ++r) gt[(kk * 4 + r) * WV_C + j] = fast_tanh_w(at[r] + btanh) * fast_sigmoid_w(as[r] + bsig);
      wsync();
      const float4 gv = *(const float4 *)(gt + j * WV_C + kk * 4);
      f32x4 ar = {0.f, 0.f, 0.f, 0.f}, s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
      MFMA4(ar, gv, P.wrs[0]);
      MFMA4(s0, gv, P.wrs[1]);
      MFMA4(s1, gv, P.wrs[2]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (has_res) x[mi][r] = fmaxf(ar[r] + bres, 0.f) + x[mi][r];
        skip[mi][0][r] = skip[mi][0][r] + fmaxf(s0[r] + bsk0, 0.f);
        skip[mi][1][r] = skip[mi][1][r] + fmaxf(s1[r] + bsk1, 0.f);
      }
      wsync();
    }
  };
  for (int blk = 0; blk < a.NB; blk += 2) {
    run_block(blk, pb[0], pb[1]);
    if (blk + 1 < a.NB) run_block(blk + 1, pb[1], pb[0]);
  }
  __syncthreads();


  } else {
    // ---- split-bf16 block loop (transposed: lane = time column n = lane & 15, rows = channels 4 kk + r).
    //      LDS: u for the delayed taps only, [plane hi | lo][2 buffers][4 channel groups kk][WV_T + WV_PAD rows][4 x bf16]:
    //      16 lanes of one kk touch 128 contiguous bytes and the kk chunks sit 128 bytes apart mod 256, so the 8-byte
    //      accesses are conflict-free at the full ds_read_b64 rate (2 LDS cycles per wave-instruction; right after the
    //      barrier all 12 waves fetch their delayed taps at once and that burst is on every wave's critical path).  One
    //      address add per block: the four reads (rows t - 2d and t - d, hi and lo) are immediate offsets from it.
    // LDS instruction ORDER is part of the design (a wave's LDS operations complete in issue order): BatchNorm vectors, the
    // u write, the gate operands - barrier - the delayed taps, and only then the res | skip operands, which are not needed
    // for another ~600 cycles (requested after the tap MFMAs instead: no gain, measured).  The wait in front of the barrier is counted (only the u write has to be complete), so
    // nobody waits at the barrier for 14 KB of operands per wave to stream out of LDS.
    // 12 / NW row tiles per wave (template parameter): every statement of the block body runs over the wave's tiles, so a
    // wave with several tiles issues independent MFMAs / gate evaluations back to back.
    // The loop is bound by vector-instruction ISSUE (each of the 3 waves of a SIMD issues its ~80 vector instructions per
    // block, and every bf16 MFMA holds the SIMD's vector issue for 8 of its 16 cycles), so the block body carries no
    // instruction it can avoid: ReLU is one v_max (fmaxf costs a canonicalising v_max in front), the exp2 scale factors
    // of the gates sit in the packed weights, the dilation comes out of two SGPR pairs read before the loop.
    constexpr int U_KK_B = (WV_T + WV_PAD) * 8, U_BUF_B = 4 * U_KK_B, U_PLANE_B = 2 * U_BUF_B;   // bytes
    static_assert(2 * U_PLANE_B == 2 * (WV_T + WV_PAD) * WV_C * 4, "u planes must fill exactly the fp32 u buffers' bytes");
    static_assert(U_KK_B % 256 == 128, "the two channel groups of a 32-lane read group must sit 128 bytes apart (mod 256): conflict-free ds_read_b64");
    unsigned char *ldsb = (unsigned char *)lds;
    const unsigned lds0 = (unsigned)(uintptr_t)lds;  // low 32 bits of a flat LDS pointer = the LDS byte address
    for (int i = tid; i < 2 * 2 * 4 * WV_PAD; i += WV_THREADS) {                  // causal zero rows: [plane][buffer][kk][row < PAD]
      const int pl = i / (2 * 4 * WV_PAD), b = (i / (4 * WV_PAD)) & 1, k = (i / WV_PAD) & 3, r = i % WV_PAD;
      *(uint2 *)(ldsb + pl * U_PLANE_B + b * U_BUF_B + k * U_KK_B + r * 8) = make_uint2(0u, 0u);
    }
    // this wave's tiles are consecutive: tile mi starts 16 rows = 128 bytes behind tile mi - 1 in every plane
    const int t0 = wave * WV_MPW * 16;
    const int ub = kk * U_KK_B + (WV_PAD + t0 + j) * 8;                           // this lane's (row t of tile 0, channel group kk), hi plane
    // Block parameters (14 A-operand slots = one 14 KB "page") are identical for all waves: the workgroup
    // fetches page b+2 at the top of block b and parks it in LDS at the end of the block (three buffers).  The barrier of
    // block b+1 publishes it, so in block b+2 every wave may read its operands BEFORE that block's barrier.
    // (Per-wave register prefetch cost 1 us per block: the loads can only be issued once the registers are free, i.e. late;
    // double-buffered pages read after the barrier left ~1000 cycles of operand reads on the critical path.)
    uint4 *pages = (uint4 *)(lds + WV_U_F);                                         // [3][WV_PAGE_U4]
    const uint4 *gpage = a.wpk;
    auto pclamp = [&](int q) { return tid + q * WV_THREADS < WV_PAGE_U4 ? tid + q * WV_THREADS : WV_PAGE_U4 - 1; };
    const int pidx0 = pclamp(0), pidx1 = pclamp(1), pidx2 = pclamp(2), pidx3 = pclamp(3);
#pragma unroll
    for (int q = 0; q < NPL; ++q) {  // pages 0 and 1: on their way since the top of the kernel
      const int i = tid + q * WV_THREADS;
      if (i < WV_PAGE_U4) {
        *(u32x4 *)(pages + i) = pg0[q];
        *(u32x4 *)(pages + WV_PAGE_U4 + i) = pg1[q];
      }
    }
    // The BatchNorm vectors are needed BEFORE a block's barrier (they produce u), i.e. before that block's
    // page is published: all blocks' copies live in their own small table, filled once.
    float4 *bnall = (float4 *)(lds + WV_U_F + WV_PG_F);                                // [NB][2][4] float4 = scale, shift
    if (tid < a.NB * 8) *(f32x4 *)(bnall + tid) = bnv;
    __syncthreads();
    const unsigned long long dil_lo = a.dil4[0], dil_hi = a.dil4[1];             // kernel-argument SGPRs: no load inside the loop
    const short one = (short)(kk == 0 ? 0x3F80 : 0);
    const s16x4 one2 = {one, one, 0, 0};                                          // k-slots 4, 5 of lane group 0 = 1.0: the bias slots (hi, lo)
    int pbuf = 0;  // blk % 3
    for (int blk = 0; blk < a.NB; ++blk) {
      const int bo = (blk & 1) * U_BUF_B;
      const int d = (int)(((blk < 16 ? dil_lo : dil_hi) >> (4 * (blk & 15))) & 15);
      const int nblk = blk + 2 < a.NB ? blk + 2 : a.NB - 1;                      // unconditional prefetch target
      // (named registers, not an array: the array form stayed in scratch memory and every block waited for its own prefetch)
      const uint4 *gnext = gpage + (size_t)nblk * WV_PAGE_U4;
      uint4 np0 = gnext[pidx0], np1 = gnext[pidx1], np2 = np0, np3 = np0;
      if (NPL > 2) np2 = gnext[pidx2];
      if (NPL > 3) np3 = gnext[pidx3];
      __builtin_amdgcn_sched_barrier(0);  // keep the loads HERE (the scheduler would sink them to their use)
      const uint4 *pg = pages + pbuf * WV_PAGE_U4;
      const bf16x8 *wsl = (const bf16x8 *)pg + lane;                             // slot q: wsl[q * 64]
      const float4 bn_s = bnall[blk * 8 + kk], bn_t = bnall[blk * 8 + 4 + kk];
      // BatchNorm affine (wavenet_model.py:57): a tile's u = the undelayed tap's B operand
      s16x4 u2h[WV_MPW], u2l[WV_MPW];
      const unsigned wa = lds0 + (unsigned)(bo + ub);
#pragma unroll
      for (int mi = 0; mi < WV_MPW; ++mi) {
        const float uv[4] = {x[mi][0] * bn_s.x + bn_t.x, x[mi][1] * bn_s.y + bn_t.y, x[mi][2] * bn_s.z + bn_t.z, x[mi][3] * bn_s.w + bn_t.w};
        split4(uv, u2h[mi], u2l[mi]);
      }
      // hi and lo planes straight from the operand register pairs (immediate offsets: tile, plane)
#define WV_WR(mi_)                                                                                                   \
  if ((mi_) < WV_MPW)                                                                                                \
    asm volatile("ds_write_b64 %0, %1 offset:%3\n\tds_write_b64 %0, %2 offset:%4"                                   \
                 : : "v"(wa), "v"(u2h[(mi_) < WV_MPW ? (mi_) : 0]), "v"(u2l[(mi_) < WV_MPW ? (mi_) : 0]), "n"((mi_) * 128), "n"(U_PLANE_B + (mi_) * 128) : "memory");
      WV_WR(0) WV_WR(1) WV_WR(2)
#undef WV_WR
      // this block's gate operands (the page was published one barrier ago)
      const bf16x8 w0 = wsl[0 * 64], w1 = wsl[1 * 64], w2 = wsl[2 * 64], w3 = wsl[3 * 64];
      const bf16x8 w4 = wsl[4 * 64], w5 = wsl[5 * 64], w6 = wsl[6 * 64], w7 = wsl[7 * 64];
      // k-step 0 = tap 2, operands in registers - these MFMAs run while the other waves arrive.  The 8 k-slots of a lane
      // group hold TWO 4-channel groups: (w_hi | w_hi) x (u_hi | u_lo) is hi*hi + hi*lo in one MFMA, (w_lo | bias) x (u_hi | 1, 1)
      // the lo*hi product plus the bias (hi and lo halves in k-slots 4, 5 of lane group 0): model_pack.h, pack_wave
      f32x4 as[WV_MPW], at[WV_MPW];
#pragma unroll
      for (int mi = 0; mi < WV_MPW; ++mi) {
        as[mi] = (f32x4){0.f, 0.f, 0.f, 0.f};
        at[mi] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const bf16x8 xua = cat8(u2h[mi], u2l[mi]), xub = cat8(u2h[mi], one2);
        MFMA_BF(as[mi], w0, xua); MFMA_BF(at[mi], w2, xua);
        MFMA_BF(as[mi], w1, xub); MFMA_BF(at[mi], w3, xub);
      }
      // u complete (all rows, all waves).  At most the 8 operand reads above are younger than the u writes, so "at most 8
      // LDS operations outstanding" means the writes have landed; the operands keep streaming across the barrier.
      asm volatile("s_waitcnt lgkmcnt(8)\n\ts_barrier" ::: "memory");
      // k-step 1 = (tap 0 | tap 1) = rows t - 2d and t - d (rows < 0 hit the zero pad, d <= 8)
      s16x4 u0h[WV_MPW], u1h[WV_MPW], u0l[WV_MPW], u1l[WV_MPW];
      {
        const unsigned ra = wa - 16u * (unsigned)d;
#define WV_RD4(mi_, d_)                                                                                                     \
  if ((mi_) < WV_MPW)                                                                                                       \
    asm volatile("ds_read_b64 %0, %4 offset:%5\n\tds_read_b64 %1, %4 offset:%6\n\tds_read_b64 %2, %4 offset:%7\n\tds_read_b64 %3, %4 offset:%8" \
                 : "=&v"(u0h[(mi_) < WV_MPW ? (mi_) : 0]), "=&v"(u1h[(mi_) < WV_MPW ? (mi_) : 0]),                           \
                   "=&v"(u0l[(mi_) < WV_MPW ? (mi_) : 0]), "=&v"(u1l[(mi_) < WV_MPW ? (mi_) : 0])                            \
                 : "v"(ra), "n"((mi_) * 128), "n"((mi_) * 128 + 8 * (d_)), "n"(U_PLANE_B + (mi_) * 128),                     \
                   "n"(U_PLANE_B + (mi_) * 128 + 8 * (d_))                                                                  \
                 : "memory");
#define WV_RD(d_) WV_RD4(0, d_) WV_RD4(1, d_) WV_RD4(2, d_)
        if (d == 1) { WV_RD(1) }
        else if (d == 2) { WV_RD(2) }
        else if (d == 4) { WV_RD(4) }
        else if (d == 8) { WV_RD(8) }
        else {  // any other dilation: plain loads
#pragma unroll
          for (int mi = 0; mi < WV_MPW; ++mi) {
            const unsigned char *base = ldsb + bo + ub + mi * 128;
            u0h[mi] = *(const s16x4 *)(base - 16 * d); u1h[mi] = *(const s16x4 *)(base - 8 * d);
            u0l[mi] = *(const s16x4 *)(base + U_PLANE_B - 16 * d); u1l[mi] = *(const s16x4 *)(base + U_PLANE_B - 8 * d);
          }
        }
#undef WV_RD
#undef WV_RD4
      }
      // res | skip operands: behind the taps in the LDS queue, in front of their use by a whole gate evaluation
      const bf16x8 r0 = wsl[8 * 64], r1 = wsl[9 * 64], r2 = wsl[10 * 64], r3 = wsl[11 * 64], r4 = wsl[12 * 64], r5 = wsl[13 * 64];
      // the taps (6 younger reads may be in flight)
#pragma unroll
      for (int mi = 0; mi < WV_MPW; ++mi)
        asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(u0h[mi]), "+v"(u1h[mi]), "+v"(u0l[mi]), "+v"(u1l[mi]) : : "memory");
#pragma unroll
      for (int mi = 0; mi < WV_MPW; ++mi) {
        const bf16x8 xdh = cat8(u0h[mi], u1h[mi]), xdl = cat8(u0l[mi], u1l[mi]);
        MFMA_BF(as[mi], w4, xdh); MFMA_BF(at[mi], w6, xdh);
        MFMA_BF(as[mi], w5, xdh); MFMA_BF(at[mi], w7, xdh);
        MFMA_BF(as[mi], w4, xdl); MFMA_BF(at[mi], w6, xdl);
      }
      // gate: tanh(t) * sigmoid(s); biases AND the exp2 scale factors (-log2 e, 2 log2 e) are inside the accumulators
      f32x4 ar[WV_MPW], s0[WV_MPW], s1[WV_MPW];
#pragma unroll
      for (int mi = 0; mi < WV_MPW; ++mi) {
        float gv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float et = __builtin_amdgcn_exp2f(at[mi][r]);    // exp(2 t): inf -> tanh 1, 0 -> -1
          const float es = __builtin_amdgcn_exp2f(as[mi][r]);    // exp(-s)
          gv[r] = (1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + et)) * __builtin_amdgcn_rcpf(1.0f + es);
        }
        s16x4 g_h, g_l;
        split4(gv, g_h, g_l);  // the gate product is the res / skip conv's B operand as it stands
        ar[mi] = (f32x4){0.f, 0.f, 0.f, 0.f}; s0[mi] = ar[mi]; s1[mi] = ar[mi];
        const bf16x8 ga8 = cat8(g_h, g_l), gb8 = cat8(g_h, one2);
        MFMA_BF(ar[mi], r0, ga8); MFMA_BF(s0[mi], r2, ga8); MFMA_BF(s1[mi], r4, ga8);
        MFMA_BF(ar[mi], r1, gb8); MFMA_BF(s0[mi], r3, gb8); MFMA_BF(s1[mi], r5, gb8);
      }
      // residual / skip update; biases ride in the MFMA, and a block without a residual conv has zero
      // res weights and bias (relu(0) = 0), so no special case
#pragma unroll
      for (int mi = 0; mi < WV_MPW; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x[mi][r] = relu1(ar[mi][r]) + x[mi][r];
          skip[mi][0][r] = skip[mi][0][r] + relu1(s0[mi][r]);
          skip[mi][1][r] = skip[mi][1][r] + relu1(s1[mi][r]);
        }
      // park page blk+2 (loaded a whole block ago) in the buffer that held page blk-1: every wave is past its
      // reads of that one (they precede the barrier of block blk, which everyone here has passed)
      const int nbuf = pbuf == 0 ? 2 : pbuf - 1;  // (blk + 2) % 3
      uint4 *pn = pages + nbuf * WV_PAGE_U4;
      pn[pidx0] = np0;
      if (tid + WV_THREADS < WV_PAGE_U4) pn[pidx1] = np1;
      if (NPL > 2 && tid + 2 * WV_THREADS < WV_PAGE_U4) pn[pidx2] = np2;
      if (NPL > 3 && tid + 3 * WV_THREADS < WV_PAGE_U4) pn[pidx3] = np3;
      pbuf = pbuf == 2 ? 0 : pbuf + 1;
    }
    __syncthreads();
  }
  }
  // ---- encoder output (optional) + detect head
  if (a.enc) {
    float *e = a.enc + (size_t)w * T * WV_S;
#pragma unroll
    for (int mi = 0; mi < WV_MPW; ++mi) {
      if (TRANSPOSED) {  // transposed state: lane = time column, four consecutive channels per register quad
        const int t = (wave * WV_MPW + mi) * 16 + j;
        if (t < T) wv_enc_store_t(e + (size_t)t * WV_S, kk, skip[mi]);
        continue;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = (wave * WV_MPW + mi) * 16 + kk * 4 + r;
        if (t < T) {
          e[(size_t)t * WV_S + j] = skip[mi][0][r];
          e[(size_t)t * WV_S + 16 + j] = skip[mi][1][r];
        }
      }
    }
  }
  wv_head_w hw;
  WV_SET_VIEW(ah, wv_set_move_head)
  wv_head_load(ah, j, kk, hw);
  float best = -INFINITY;
#pragma unroll
  for (int mi = 0; mi < WV_MPW; ++mi) {
    const int t0 = (wave * WV_MPW + mi) * 16;
    const f32x4 y = wv_head_tile<TRANSPOSED>(skip[mi], hbuf + t0 * WV_S, hw, j, kk);  // [16][32] tile, wave-private
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = t0 + kk * 4 + r;
      if (t < T) best = fmaxf(best, y[r] + hw.b2);
    }
  }
  // GlobalMaxPooling1D over time: reduce over kk (lanes j, j+16, j+32, j+48), then over waves
  best = fmaxf(best, __shfl_xor(best, 16));
  best = fmaxf(best, __shfl_xor(best, 32));
  if (lane < 16) red[wave][lane] = best;
  __syncthreads();
  if (tid < 16) {
    float v = red[0][tid];
#pragma unroll
    for (int q = 1; q < WV_NW; ++q) v = fmaxf(v, red[q][tid]);
    const float p = wv_softmax16(v, tid, a.NOUT);
    WV_POST_STORE(a.tag, a.out, a.NOUT, w, 0, tid, p);
  }
}

// ---- the sequence form (fp32): a mel sequence of ANY length, evaluated as the reference's Keras model evaluates it with
//      timesteps=None - causal taps read zeros in front of row 0 and nothing else is padded - instead of as 182-row windows that
//      each pad their own left edge.  One workgroup walks one SEGMENT (wv_seg: rows [row0, row0 + n) of one sequence) in chunks of
//      NW x 16 rows through the block body of wavenet_kernel (wv_block_t: the same instructions, so row t carries the bits of
//      position T - 1 of the window that ends at t).  What a window form cannot have is carried from chunk to chunk in LDS: per
//      block the last WV_PAD = 16 rows of u (2 d <= 16), 1 KB x NB = 24 KB - they take the place of the causal zero rows, so no row
//      is computed twice.  A long sequence is cut into segments that run in parallel; a segment that does not start at row 0 of its
//      sequence starts RF - 1 rows early (RF = 1 + 2 sum d, the receptive field) from an all-zero history and discards those rows
//      (`skip`): row t depends on rows t - RF + 1 .. t only, so what it keeps are the bits of the uncut evaluation.
//      Outputs per kept row: the skip sum (enc) and the head's logits BEFORE the max over time; the pooled maxima and the
//      softmax are wave_pool_*_kernel's (sequences) or the tail of this kernel (STREAM).
//      STREAM (NW = 1): one workgroup = one stream's tick of 1..2 new rows.  The history comes from and returns to the stream's
//      state in memory; the new logit rows go into the stream's ring of the last P rows, and each new row's posterior -
//      softmax(max over the ring's rows up to it) - leaves as a tag or a row of `out` when the segment's emit bit is set.
//      FEED (ww_stream_feed): a segment of the rows a call brought for one stream (wv_feed_seg).  `mel` is the call's row buffer.
//      The stream's first segment takes its history from the stream's state, its last one returns it there.  NW = 1: a stream
//      that brought up to 16 rows - the tick's tail for rows 0 .. n - 1 of the tile (register r of lane group kk is row 4 kk + r),
//      every row's posterior to `post`.  NW = 12: more rows, logits to `logits`; wave_feed_pool_kernel / wave_feed_ring_kernel
//      are its tail.
struct wave_seq_args {
  const wv_seg *segs;
  float *enc, *logits;          // [mel rows][32], [mel rows][NOUT]: a segment's kept rows, by mel row; either may be NULL
  // STREAM
  const int64_t *win_row;       // [nw] first new mel row (in `mel` = the bank's mirrored rings)
  const int32_t *win_valid;     // [nw] new rows (1..2)
  const int32_t *win_aux;       // [nw] stream | emit << 16
  float *state;                 // [S][NB][4 kk][WV_PAD][4]
  float *zring;                 // [S][P][16]
  int32_t *zpos;                // [S][2]: the ring slot of the next row, rows held (<= P)
  float *out;                   // [2 S][NOUT] (no tags)
  int P;
  // FEED
  const wv_feed_seg *fsegs;     // [workgroups]
  float *post;                  // [rows of the call]: the posterior column of every new row (the one-wave form's tail)
  // (SET, whole sequences - ww_set_wave_sequence*: enc / logits are [planes][a.wa.mel_rows][...], workgroup (x, y) writes plane y)
};

// A stream's ring of its last P logit rows [P][16] and zpos = {the slot of the next row, rows held (<= P)}: the slot of the row
// `off` rows from the next one (off >= -P), and the advance by n rows
__device__ __forceinline__ int wv_ring_slot(int pos, int off, int P) { return (pos + off + P) % P; }
__device__ __forceinline__ void wv_zpos_advance(int32_t *zpos, int sid, int pos, int held, int n, int P) {
  zpos[2 * sid] = (pos + n) % P;
  zpos[2 * sid + 1] = held + n < P ? held + n : P;
}

// The tail of the one-wave forms (ROWS_: 2, a tick, or 16, a feed).  The tile's first n_ <= ROWS_ rows are a stream's new logit rows (y_: register r of lane group kk_
// is row 4 kk_ + r, without the last bias b2_): the pooled maximum over the ring's rows up to each new row, the softmax - SINK_, a
// statement, gets new row k's posterior p in lanes 0..15, lane c = column c - then the ring and its position.  zl_: [ROWS_][16]
// floats of LDS.  (A macro: as a function template taking the sink as a callable it moved instructions in both kernels.)
#define WV_RING_TAIL(ROWS_, q_, sid_, n_, y_, b2_, zl_, lane_, j_, kk_, NOUT_, SINK_)                                            \
  do {                                                                                                                           \
    if ((ROWS_) == 2) { /* (written out: as the r-loop below under `4 kk + r < 2` the tick's kernel was scheduled otherwise) */  \
      if ((kk_) == 0) {                                                                                                          \
        (zl_)[(j_)] = (y_)[0] + (b2_);                                                                                           \
        (zl_)[16 + (j_)] = (y_)[1] + (b2_);                                                                                      \
      }                                                                                                                          \
    } else {                                                                                                                     \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) (zl_)[((kk_) * 4 + r) * 16 + (j_)] = (y_)[r] + (b2_);                        \
    }                                                                                                                            \
    wsync();                                                                                                                     \
    const int P = (q_).P, pos = (q_).zpos[2 * (sid_)], held = (q_).zpos[2 * (sid_) + 1];                                         \
    float *ring = (q_).zring + (size_t)(sid_) * P * 16;                                                                          \
    for (int k = 0; k < (n_); ++k) {                                                                                             \
      const int cnt = held + k + 1 < P ? held + k + 1 : P; /* rows of the pool that ends at new row k */                         \
      float m = -INFINITY;                                                                                                       \
      for (int i = (kk_); i < cnt; i += 4) { /* i rows back from it: a new row, or the ring's */                                 \
        const float v = i <= k ? (zl_)[(k - i) * 16 + (j_)] : ring[(size_t)wv_ring_slot(pos, k - i, P) * 16 + (j_)];             \
        m = fmaxf(m, v);                                                                                                         \
      }                                                                                                                          \
      m = fmaxf(m, __shfl_xor(m, 16));                                                                                           \
      m = fmaxf(m, __shfl_xor(m, 32));                                                                                           \
      if ((lane_) < 16) {                                                                                                        \
        const float p = wv_softmax16(m, lane_, NOUT_);                                                                           \
        SINK_;                                                                                                                   \
      }                                                                                                                          \
    }                                                                                                                            \
    /* the ring is read before it is written: a tick's new row 1 takes the slot of the oldest row of new row 0's pool (a feed's */ \
    /* n <= 16 < P: a new row never takes the slot of another new row) */                                                        \
    wsync();                                                                                                                     \
    if ((lane_) < 16)                                                                                                            \
      for (int k = 0; k < (n_); ++k) ring[(size_t)((pos + k) % P) * 16 + (lane_)] = (zl_)[k * 16 + (lane_)];                     \
    if ((lane_) == 0) wv_zpos_advance((q_).zpos, sid_, pos, held, n_, P);                                                        \
  } while (0)

// SET (a causal bank created from a model set): the member of the workgroup's stream, set.ids[sid].
// SET, whole sequences (a set's ww_set_wave_sequence*): workgroup (x, y) is segment x into output plane y.  Its member is
// set.ids[y] - every sequence by the call's slot y - or, where set.aux is given (one plane, gridDim.y = 1), set.ids[set.aux[x]]:
// aux[x] is the sequence of segment x and ids holds one member per sequence.  The segment table is the single model's.
// ALL (a feed of an every-member bank, ww_stream_feed_all): workgroup (x, y) is segment x run by member slot y of gridDim.y.  The
// segment table and the row buffer are the physical streams'; the workgroup's weights, history, logit ring and position are those of
// VIRTUAL stream sid K + y, and its logits and posteriors go to plane y of q.logits / q.post ([K][a.wa.mel_rows][...]).  Slot and K
// are the grid's, i.e. scalars: nothing is added to a lane's registers.
template <int NW, bool STREAM, bool FEED = false, bool SET = false, bool ALL = false>
__global__ __launch_bounds__(NW * 64, NW == 12 ? 3 : 1) void wavenet_seq_kernel(wave_args a, wave_seq_args q, ww_set_ref set) {
  static_assert(!SET || STREAM || FEED || NW == 12, "whole sequences run the twelve-wave form");
  static_assert(!ALL || (SET && FEED), "every member slot on a segment: the feed of a bank created from a model set");
  if constexpr (ALL) {
    const int slot = blockIdx.y, K = gridDim.y;
    const int v = __builtin_amdgcn_readfirstlane(q.fsegs[blockIdx.x].sid) * K + slot;
    if (q.logits) q.logits += (size_t)slot * a.wa.mel_rows * a.NOUT;
    q.post += (size_t)slot * a.wa.mel_rows;
    const long long off = ww_set_offset(set, v);
    wv_set_move_front(a, off);
    wv_set_move_blocks(a, off);
    wv_set_move_head(a, off);
  } else if constexpr (SET) {
    [[maybe_unused]] int slot = 0;
    if constexpr (!STREAM && !FEED) {
      const int plane = blockIdx.y;
      slot = set.aux ? __builtin_amdgcn_readfirstlane(set.aux[blockIdx.x]) : plane;
      if (q.enc) q.enc += (size_t)plane * a.wa.mel_rows * WV_S;  // (a plane has a row per row of the mel buffer)
      if (q.logits) q.logits += (size_t)plane * a.wa.mel_rows * a.NOUT;
    }
    const long long off = ww_set_offset(set, FEED ? q.fsegs[blockIdx.x].sid : STREAM ? q.win_aux[blockIdx.x] & 0xffff : slot);
    wv_set_move_front(a, off);
    wv_set_move_blocks(a, off);
    wv_set_move_head(a, off);
  }
  static_assert(!(STREAM && FEED) && (!FEED || NW == 1 || NW == 12), "a feed is not a tick; its forms are one wave and twelve");
  constexpr int CH = NW * 16, THREADS = NW * 64, UPL = (CH + WV_PAD) * 4;
  constexpr int U_F = 2 * 4 * UPL, H_F = CH * WV_S, IN_F = CH * WV_INLD, V_F = WV_VT_F, HB = 4 * WV_PAD * 4;
  static_assert(UPL % 64 == 0, "u planes must start on the same bank");
  static_assert(IN_F <= U_F + H_F, "the staged input lies under the u buffers and the head tile");
  static_assert(!STREAM || NW == 1, "a stream's tick is one tile");
  // [ u[2][4][UPL] | head tile [CH][32] ] (the staged input [CH][48] under both) | vector table (WV_VT_F) | history [32][HB]
  __shared__ __align__(16) float lds[U_F + H_F + V_F + 32 * HB];
  float *ubuf = lds, *hbuf = lds + U_F, *vtab = hbuf + H_F, *hist = vtab + V_F, *in_lds = lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kk = lane >> 4;
  const int w = blockIdx.x;
  int64_t row0;
  int n, skipn, sid = 0, emit = 0, fflags = 0;
  if (FEED) {
    const wv_feed_seg sg = q.fsegs[w];
    row0 = sg.row0; n = sg.n; skipn = sg.skip; sid = sg.sid; fflags = sg.flags;
    if constexpr (ALL) sid = __builtin_amdgcn_readfirstlane(sid) * (int)gridDim.y + (int)blockIdx.y;  // the virtual stream
  } else if (STREAM) {
    row0 = q.win_row[w];
    n = q.win_valid[w];
    n = n < CH ? n : CH;
    skipn = 0;
    const int aux = q.win_aux[w];
    sid = aux & 0xffff;
    emit = aux >> 16;
  } else {
    const wv_seg sg = q.segs[w];
    row0 = sg.row0; n = sg.n; skipn = sg.skip;
  }
  // (SET: the twelve-wave feed form, at the register limit of three waves per SIMD, came out one register over it with tid held
  //  across the block loop.  Its later readers form tid again instead: the wave's first thread, kept as a scalar, plus the lane
  //  number from mbcnt - through an empty asm, so that each reader's copy is a value of its own and not one hoisted to the top)
  [[maybe_unused]] int s_wave0 = 0;
  if constexpr (SET) s_wave0 = __builtin_amdgcn_readfirstlane(tid & ~63);
  auto tid_again = [&]() -> int {
    if constexpr (SET) {
      int base = s_wave0;
      asm volatile("" : "+s"(base));
      return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)base));
    } else {
      return tid;
    }
  };
  for (int i = tid; i < a.NB * WV_VT_BLK; i += THREADS) {  // all blocks' small vectors
    WV_VT_FETCH(vtab[i], a, i);
  }
  {
    const f32x4 *sp = (const f32x4 *)(q.state + (size_t)sid * a.NB * HB);
    for (int i = tid; i < a.NB * HB / 4; i += THREADS) ((f32x4 *)hist)[i] = (STREAM || (FEED && (fflags & 1))) ? sp[i] : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const bool vec_in = (a.n_mel & 3) == 0 && ((((uintptr_t)a.mel) & 15) == 0);
  f32x4 y = {0.f, 0.f, 0.f, 0.f};
  float b2 = 0.f;
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int valid = n - c0 < CH ? n - c0 : CH;
    // (the thread's coordinates as values the compiler cannot move out of the chunk loop: the per-lane addresses of the staging,
    //  the input conv and - formed again behind the block loop - the head would otherwise be held, i.e. spilled, across the block
    //  loop, which runs at the register limit of three waves per SIMD)
    int tc = tid_again();
    asm volatile("" : "+v"(tc));
    const int wc = tc >> 6, jc = tc & 15, kc = (tc >> 4) & 3;
    const int tl = wc * 16 + jc;  // this lane's time column in the chunk
    // the input conv's operands: requested now, used behind the staging (per chunk: they are not held across the block loop)
    float4 bw[3];
#pragma unroll
    for (int kb = 0; kb < 3; ++kb) bw[kb] = *(const float4 *)(a.w_in4 + (unsigned)((kb * 4 + kc) * 16 + jc) * 4);
    __syncthreads();  // the chunk before is through with the head tile (and, the first time, the tables are in place)
    // ---- stage the chunk: in_lds[t][0..47], zero outside [0, valid) x [0, n_mel)
    const float *src = a.mel + (row0 + c0) * a.n_mel;
    if (vec_in) {
      for (int i = tc; i < CH * (WV_INLD / 4); i += THREADS) {
        const int t = i / (WV_INLD / 4), c = (i - t * (WV_INLD / 4)) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t < valid && c < a.n_mel) v = *(const f32x4 *)(src + (size_t)t * a.n_mel + c);
        *(f32x4 *)(in_lds + t * WV_INLD + c) = v;
      }
    } else {
      for (int i = tc; i < CH * WV_INLD; i += THREADS) {
        const int t = i / WV_INLD, c = i - t * WV_INLD;
        in_lds[i] = (t < valid && c < a.n_mel) ? src[(size_t)t * a.n_mel + c] : 0.f;
      }
    }
    __syncthreads();
    // ---- input 1x1 conv + ReLU -> x, transposed (lane = time column, registers = channels 4 kk + r): wavenet_kernel's
    f32x4 x[1], skip[1][2];
    WV_INPUT_TILE(true, in_lds, tl, kc, bw, a.b_in, 0.f, x[0], skip[0]);
    wv_wblk pw[2];
    wv_wload(a, 0, jc, kc, pw[0]);
    __syncthreads();  // in_lds is dead from here on
    WV_BLOCKS_T(1, UPL, true, (SET ? 1 : 0), a, ubuf, vtab, jc, kc, tl, x, skip, pw, hist, valid, wc == 0);
    // ---- a kept row's skip sum and logits
    int td = tid_again();
    asm volatile("" : "+v"(td));
    const int wd = td >> 6, jd = td & 15, kd = (td >> 4) & 3;
    const int ts = c0 + wd * 16 + jd;  // this lane's time column, in rows of the segment
    if (q.enc && ts >= skipn && ts < n) wv_enc_store_t(q.enc + (size_t)(row0 + ts) * WV_S, kd, skip[0]);
    wv_head_w hw;
    wv_head_load(a, jd, kd, hw);
    y = wv_head_tile<true>(skip[0], hbuf + wd * 16 * WV_S, hw, jd, kd);  // (wave-private tile: no barrier)
    b2 = hw.b2;
    if (!STREAM && q.logits && jd < a.NOUT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = c0 + wd * 16 + kd * 4 + r;
        if (t >= skipn && t < n) q.logits[(size_t)(row0 + t) * a.NOUT + jd] = y[r] + b2;
      }
    }
  }
  if (STREAM) {  // the tick's n <= 2 new rows; a posterior leaves, as a tag or a row of `out`, when the segment's emit bit is set
    WV_RING_TAIL(2, q, sid, n, y, b2, hbuf, lane, j, kk, a.NOUT, if (emit) WV_POST_STORE(a.tag, q.out, a.NOUT, 2 * sid, k, lane, p));
  }
  if (FEED && NW == 1) {  // the n <= 16 new rows of the tile; every row's posterior leaves
    WV_RING_TAIL(16, q, sid, n, y, b2, hbuf, lane, j, kk, a.NOUT, if (lane == a.tag.pidx) q.post[row0 + k] = p);
  }
  if (STREAM || (FEED && (fflags & 2))) {  // the history returns to the stream's state (a feed: from the stream's last segment)
    __syncthreads();
    f32x4 *sp = (f32x4 *)(q.state + (size_t)sid * a.NB * HB);
    for (int i = tid_again(); i < a.NB * HB / 4; i += THREADS) sp[i] = ((const f32x4 *)hist)[i];
  }
}

// ---- the tail of a feed's twelve-wave form.  The pool of new row k of a stream ends at k and covers the last P rows of
//      [the ring's held rows | the new rows].  One workgroup per 256 new rows: the rows and the P - 1 in front of them in LDS
//      (-inf where the stream has no row yet), sixteen lanes per row (lane c = column c), the maximum - exact in any order - and
//      the tick's softmax.  The ring is only read here: wave_feed_ring_kernel writes it, behind this kernel.
__global__ __launch_bounds__(256) void wave_feed_pool_kernel(const float *z, const wv_feed_pool *tab, int NOUT, int P, int pidx,
                                                             const float *zring, const int32_t *zpos, float *post) {
  extern __shared__ __align__(16) float pool_tile[];  // [WW_FEED_POOL_ROWS + P - 1][16]
  const wv_feed_pool d = tab[blockIdx.x];
  const int tid = threadIdx.x, c = tid & 15, g = tid >> 4;
  const int pos = zpos[2 * d.sid], held = zpos[2 * d.sid + 1];
  const float *ring = zring + (size_t)d.sid * P * 16;
  const int here = d.n - d.k0 < WW_FEED_POOL_ROWS ? d.n - d.k0 : WW_FEED_POOL_ROWS;
  for (int i = g; i < here + P - 1; i += 16) {
    const int64_t v = (int64_t)d.k0 - (P - 1) + i;  // the row, counted from the stream's first new row
    float x = -INFINITY;
    if (c < NOUT) {
      if (v >= 0) x = z[(d.row0 + v) * NOUT + c];
      else if (v >= -held) x = ring[(size_t)wv_ring_slot(pos, (int)v, P) * 16 + c];
    }
    pool_tile[i * 16 + c] = x;
  }
  __syncthreads();
  for (int r = g; r < here; r += 16) {
    float m = -INFINITY;
    for (int i = 0; i < P; ++i) m = fmaxf(m, pool_tile[(r + i) * 16 + c]);
    const float p = wv_softmax16(m, c, NOUT);
    if (c == pidx) post[d.row0 + d.k0 + r] = p;
  }
}

// one workgroup per stream of the twelve-wave form: its last min(n, P) new logit rows into the ring, the ring's position and count
__global__ __launch_bounds__(256) void wave_feed_ring_kernel(const float *z, const wv_feed_pool *tab, int NOUT, int P, float *zring,
                                                             int32_t *zpos) {
  const wv_feed_pool d = tab[blockIdx.x];
  const int tid = threadIdx.x;
  const int pos = zpos[2 * d.sid], held = zpos[2 * d.sid + 1];
  float *ring = zring + (size_t)d.sid * P * 16;
  const int m = d.n < P ? d.n : P;
  for (int i = tid; i < m * 16; i += 256) {
    const int k = d.n - m + (i >> 4), c = i & 15;
    ring[(size_t)((pos + k) % P) * 16 + c] = c < NOUT ? z[(d.row0 + k) * NOUT + c] : 0.f;
  }
  __syncthreads();  // (every thread has read the position)
  if (tid == 0) wv_zpos_advance(zpos, d.sid, pos, held, d.n, P);
}

// ---- pooled maxima of the sequence form.  m[t] = max of z over the last P rows up to t (of t's own sequence), P = 0: from row 0.
//      By doubling: M_0 = z, M_{i+1}[t] = max(M_i[t], M_i[t - 2^i]) is the maximum over the last 2^(i+1) rows; with 2^k <= P < 2^(k+1)
//      m[t] = max(M_k[t], M_k[t - (P - 2^k)]).  A maximum is exact in any order, so neither the cuts of the main kernel nor the
//      order here can show in the result.  k + 1 passes over [rows][NOUT] floats: for 2.4 h of audio, 8 x 7 MB.
__device__ __forceinline__ int64_t wv_row_in_seq(const int64_t *offs, int n_seq, int64_t row) {
  int lo = 0, hi = n_seq;  // the sequence s with offs[s] <= row < offs[s + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offs[mid] <= row) lo = mid; else hi = mid;
  }
  return row - offs[lo];
}

// (blockIdx.y: the plane of a model set's call - `plane` floats each, the same sequences in every one; a single model's call has one)
__global__ __launch_bounds__(256) void wave_pool_step_kernel(const float *in, float *out, int64_t rows, int NOUT, const int64_t *offs, int n_seq,
                                                             int64_t step, int64_t plane) {
  // (rows = [offs[0], offs[n_seq]): rows of the buffers in front of or behind the sequences are neither read nor written)
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * NOUT) return;
  in += blockIdx.y * plane;
  out += blockIdx.y * plane;
  i += offs[0] * NOUT;
  const int64_t row = i / NOUT;
  float v = in[i];
  if (wv_row_in_seq(offs, n_seq, row) >= step) v = fmaxf(v, in[i - step * NOUT]);
  out[i] = v;
}

// sixteen lanes per row (lane c = column c): the last step of the pooled maximum and wavenet_kernel's softmax
__global__ __launch_bounds__(256) void wave_pool_final_kernel(const float *M, int64_t rows, int NOUT, const int64_t *offs, int n_seq, int64_t back,
                                                              float *pf, int64_t plane) {
  M += blockIdx.y * plane;
  pf += blockIdx.y * plane;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = offs[0] + (g >> 4), rc = row < rows ? row : rows - 1;
  const int c = (int)(g & 15);
  float v = c < NOUT ? M[rc * NOUT + c] : -INFINITY;
  if (back > 0 && c < NOUT && wv_row_in_seq(offs, n_seq, rc) >= back) v = fmaxf(v, M[(rc - back) * NOUT + c]);
  const float p = wv_softmax16(v, c, NOUT);
  if (row < rows && c < NOUT) pf[row * NOUT + c] = p;
}

// one workgroup per sequence and plane: softmax(max over all its rows) - what model(X) returns with timesteps=None
__global__ __launch_bounds__(256) void wave_seq_post_kernel(const float *z, const int64_t *offs, int NOUT, float *post, int64_t plane) {
  __shared__ float red[16][16];
  z += blockIdx.y * plane;
  post += (size_t)blockIdx.y * gridDim.x * NOUT;  // [planes][n_seq][NOUT]
  const int s = blockIdx.x, tid = threadIdx.x, c = tid & 15, g = tid >> 4;
  const int64_t r0 = offs[s], r1 = offs[s + 1];
  if (r1 <= r0) return;  // an empty sequence has no posterior: its row of `post` is left as it is
  float m = -INFINITY;
  if (c < NOUT)
    for (int64_t r = r0 + g; r < r1; r += 16) m = fmaxf(m, z[r * NOUT + c]);
  red[g][c] = m;
  __syncthreads();
  if (tid < 16) {
    float v = red[0][tid];
#pragma unroll
    for (int k = 1; k < 16; ++k) v = fmaxf(v, red[k][tid]);
    const float p = wv_softmax16(v, tid, NOUT);
    if (tid < NOUT) post[(size_t)s * NOUT + tid] = p;
  }
}

size_t ww_wave_workspace(const ww_model *, int) { return 256; }

// The model's side of wave_args, from zero.  wave_head_args: the sizes and the detect head - all ww_k_wave_detect needs, and nothing
// is refused; wave_model_args: with the encoder of every other launch - the mel buffer, weights, dilations and the residual mask.
// wave_model_args OVERWRITES `a` as a whole: a launcher calls it first and sets its own fields (wa, out, enc, tag, fe, fb) after it.
static wave_args wave_head_args(const ww_wave_dev &v) {
  wave_args a = {};
  a.T = v.T; a.n_mel = v.n_mel; a.NB = v.NB; a.NOUT = v.NOUT;
  a.d_w1_4 = v.d_w1; a.d_b1 = v.d_b1; a.d_w2_4 = v.d_w2; a.d_b2 = v.d_b2;
  return a;
}
static int wave_model_args(ww_ctx *ctx, const ww_wave_dev &v, const float *d_mel, wave_args &a) {
  if (v.NB > 32) return ww_fail(ctx, WW_EINVAL, "Wavenet with %d blocks: kernel limit 32", v.NB);
  a = wave_head_args(v);
  a.mel = d_mel;
  for (int b = 0; b < v.NB; ++b) {
    if (v.dil[b] < 1 || v.dil[b] > 8) return ww_fail(ctx, WW_EINVAL, "dilation %d of block %d outside 1..8", v.dil[b], b);
    a.dil4[b >> 4] |= (unsigned long long)v.dil[b] << (4 * (b & 15));
    if (v.has_res[b]) a.has_res_mask |= 1u << b;
  }
  a.w_in4 = v.w_in; a.b_in = v.b_in; a.bn_s = v.bn_s; a.bn_t = v.bn_t;
  a.w_gate4 = v.w_gate; a.b_gate = v.b_gate; a.w_rs4 = v.w_rs; a.b_rs = v.b_rs;
  a.wpk = (const uint4 *)v.wpk;
  return WW_OK;
}

// The arithmetic form of a model's window kernel - split-bf16, fp32 row-major (WW_OPT_WAVENET_ROWMAJOR), fp32 transposed - decided
// ONCE, and its launch.  The transposed forms run twelve waves x one tile up to wave_wide_from(m) windows per launch and four waves x
// three tiles above; the row-major loop and the one-launch tick (TICK = 1 / 2: fp32 / fp64 transform) have the twelve-wave form only.
static int wave_wide_from(const ww_model *m) { return m->precision == WW_PRECISION_BF16X3 ? WV_BF16_WIDE_FROM : WV_F32_WIDE_FROM; }
template <bool SPLIT_BF16, bool FP32T, int TICK, bool SET = false>
static void wave_launch_form(ww_ctx *ctx, int nw, bool wide, const wave_args &a, const ww_set_ref &set = ww_set_ref{}) {
  if constexpr (TICK == 0 && (SPLIT_BF16 || FP32T)) {
    if (wide) {
      hipLaunchKernelGGL((wavenet_kernel<false, SPLIT_BF16, 4, FP32T, 0, SET>), dim3(nw), dim3(4 * 64), 0, ctx->stream, a, set);
      return;
    }
  }
  hipLaunchKernelGGL((wavenet_kernel<false, SPLIT_BF16, 12, FP32T, TICK, SET>), dim3(nw), dim3(12 * 64), 0, ctx->stream, a, set);
}
template <int TICK>
static void wave_launch(ww_ctx *ctx, const ww_model *m, int nw, const wave_args &a, const ww_set_ref *set = nullptr) {
  const bool wide = nw > wave_wide_from(m);
  if (set) return wave_launch_form<false, true, TICK, true>(ctx, nw, wide, a, *set);  // (a set's view: fp32, transposed)
  if (m->precision == WW_PRECISION_BF16X3) wave_launch_form<true, false, TICK>(ctx, nw, wide, a);
  else if (m->opt_wave_rowmajor) wave_launch_form<false, false, TICK>(ctx, nw, wide, a);
  else wave_launch_form<false, true, TICK>(ctx, nw, wide, a);
}

int ww_k_wave_forward(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                      const int32_t *d_win_valid, int64_t row0, int hop, int valid_const, int nw, void *, size_t, float *d_out,
                      float *d_enc, const ww_tick_tag *tag, const ww_set_ref *set) {
  if (nw <= 0) return WW_OK;
  wave_args a;
  if (int rc = wave_model_args(ctx, m->wave, d_mel, a)) return rc;
  a.wa = {d_win_row, d_win_valid, row0, hop, valid_const, mel_rows};
  a.out = d_out; a.enc = d_enc;
  if (tag) a.tag = *tag;
  ww_launch_scope scope(ctx, m->precision == WW_PRECISION_BF16X3 ? "wavenet_kernel<bf16x3>" : "wavenet_kernel");
  // split-bf16: twelve waves x one 16-row tile while every window has a CU of its own (the 24 blocks of a window are a serial
  // chain: more waves per window cover its latencies best, 39.1 vs 45.7 us per 256 windows); from the 257th window of a launch
  // on FOUR waves x three tiles (173 registers, 74 KB: TWO workgroups per CU, each wave issuing three tiles' independent MFMAs
  // and gate evaluations back to back): 1,656 vs 1,957 us per 16,384 windows, 69.8 vs 74.5 at 512.  Same arithmetic per
  // tile in both forms: a posterior does not depend on the launch size (tests/test_gpu_parity.py).  (Six waves x two tiles -
  // also two workgroups per CU - lose at every size: 2,393 us.)
  // (round 5) fp32: the same two forms as the split-bf16 loop, the same bits in both
  wave_launch<0>(ctx, m, nw, a, set);
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

// The sequence form's reach: the fp32 transposed block loop only
int ww_wave_seq_check(ww_ctx *ctx, const ww_model *m, const char *what) {
  if (m->kind != WW_KIND_WAVENET) return ww_fail(ctx, WW_EINVAL, "%s: the sequence form exists for Wavenet models only (a CRNN's bidirectional GRUs have no causal reading)", what);
  if (m->precision != WW_PRECISION_FP32) return ww_fail(ctx, WW_EINVAL, "%s: the sequence form is fp32 only; this model is in split-bf16 mode", what);
  return WW_OK;
}

int ww_wave_receptive_field(const ww_model *m) {
  int rf = 1;
  for (int d : m->wave.dil) rf += 2 * d;
  return rf;
}

int ww_k_wave_sequence(ww_ctx *ctx, const ww_model *m, const float *d_mel, const wv_seg *d_segs, int n_segs, float *d_enc, float *d_logits,
                       const ww_set_ref *set, int planes, int64_t plane_rows) {
  if (n_segs <= 0 || planes <= 0) return WW_OK;
  if (int rc = ww_wave_seq_check(ctx, m, "ww_wave_sequence")) return rc;
  wave_args a;
  if (int rc = wave_model_args(ctx, m->wave, d_mel, a)) return rc;
  wave_seq_args q = {};
  q.segs = d_segs; q.enc = d_enc; q.logits = d_logits;
  if (set) {  // m: the set's view.  ONE launch over segments x planes
    if (planes > 65535 || (set->aux && planes != 1)) return ww_fail(ctx, WW_EINTERNAL, "ww_k_wave_sequence: %d planes in one launch", planes);
    a.wa.mel_rows = plane_rows;
    ww_launch_scope scope(ctx, "wavenet_seq_kernel<set>");
    hipLaunchKernelGGL((wavenet_seq_kernel<12, false, false, true>), dim3(n_segs, planes), dim3(12 * 64), 0, ctx->stream, a, q, *set);
    WW_HIP(ctx, hipGetLastError());
    return WW_OK;
  }
  ww_launch_scope scope(ctx, "wavenet_seq_kernel");
  hipLaunchKernelGGL((wavenet_seq_kernel<12, false>), dim3(n_segs), dim3(12 * 64), 0, ctx->stream, a, q, ww_set_ref{});
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

// pool_rows: 0 = from row 0 of each sequence.  max_len: the longest sequence.  d_a / d_b: [rows][NOUT] floats of scratch each.
// planes > 1 (a model set's call): d_z, d_a, d_b and d_pf are [planes][plane_rows][NOUT], d_post [planes][n_seq][NOUT] - the plane is
// the grid's second dimension, so the launches are those of one plane.
int ww_k_wave_pool(ww_ctx *ctx, const float *d_z, int64_t rows, int64_t row_end, int NOUT, const int64_t *d_offs, int n_seq, int64_t pool_rows,
                   int64_t max_len, float *d_a, float *d_b, float *d_pf, float *d_post, int planes, int64_t plane_rows) {
  if (rows <= 0 || n_seq <= 0 || planes <= 0) return WW_OK;  // rows: offs[n_seq] - offs[0], the rows that belong to a sequence
  if (planes > 65535) return ww_fail(ctx, WW_EINTERNAL, "ww_k_wave_pool: %d planes in one launch", planes);
  const int64_t plane = plane_rows * NOUT;
  if (d_post) {
    ww_launch_scope scope(ctx, "wave_seq_post_kernel");
    hipLaunchKernelGGL(wave_seq_post_kernel, dim3(n_seq, planes), dim3(256), 0, ctx->stream, d_z, d_offs, NOUT, d_post, plane);
    WW_HIP(ctx, hipGetLastError());
  }
  if (!d_pf) return WW_OK;
  const int64_t P = pool_rows == 0 || pool_rows > max_len ? max_len : pool_rows;  // (a pool longer than every sequence is "from row 0")
  ww_launch_scope scope(ctx, "wave_pool_kernels");
  const float *cur = d_z;
  int64_t span = 1;  // cur[t] = max over the last `span` rows
  const unsigned g1 = (unsigned)((rows * NOUT + 255) / 256);
  while (span * 2 <= P) {
    float *nxt = cur == d_a ? d_b : d_a;
    hipLaunchKernelGGL(wave_pool_step_kernel, dim3(g1, planes), dim3(256), 0, ctx->stream, cur, nxt, rows, NOUT, d_offs, n_seq, span, plane);
    cur = nxt;
    span *= 2;
  }
  hipLaunchKernelGGL(wave_pool_final_kernel, dim3((unsigned)((rows * 16 + 255) / 256), planes), dim3(256), 0, ctx->stream, cur, row_end, NOUT, d_offs, n_seq, P - span, d_pf, plane);
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

// A causal bank's tick (streams.hip): workgroup w advances stream win_aux[w] & 0xffff by its win_valid[w] new mel rows
int ww_k_wave_stream_tick(ww_ctx *ctx, const ww_model *m, const float *d_hist, const int64_t *d_win_row, const int32_t *d_win_valid,
                          const int32_t *d_win_aux, int nw, float *d_state, float *d_zring, int32_t *d_zpos, float *d_out,
                          const ww_tick_tag *tag, const ww_set_ref *set) {
  if (nw <= 0) return WW_OK;
  if (int rc = ww_wave_seq_check(ctx, m, "causal streaming tick")) return rc;
  wave_args a;
  if (int rc = wave_model_args(ctx, m->wave, d_hist, a)) return rc;
  if (tag) a.tag = *tag;
  wave_seq_args q = {};
  q.win_row = d_win_row; q.win_valid = d_win_valid; q.win_aux = d_win_aux;
  q.state = d_state; q.zring = d_zring; q.zpos = d_zpos; q.out = d_out; q.P = m->wave.T;
  ww_launch_scope scope(ctx, "wavenet_seq_kernel<stream>");
  if (set) hipLaunchKernelGGL((wavenet_seq_kernel<1, true, false, true>), dim3(nw), dim3(64), 0, ctx->stream, a, q, *set);
  else hipLaunchKernelGGL((wavenet_seq_kernel<1, true>), dim3(nw), dim3(64), 0, ctx->stream, a, q, ww_set_ref{});
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

// [slots][rows] posteriors of a feed's every-member form -> the caller's [rows][slots]
__global__ __launch_bounds__(256) void wave_feed_post_rows_kernel(const float *planes, int64_t rows, int slots, float *out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // element of out
  if (i >= rows * slots) return;
  const int64_t r = i / slots;
  const int j = (int)(i - r * slots);
  out[i] = planes[(int64_t)j * rows + r];
}

// A causal bank's feed (streams.hip: ww_stream_feed).  The forms by the rows a stream brought: up to WW_FEED_TILE_ROWS the one-wave
// form, above the twelve-wave form with its tail as two small kernels; a call may launch both.
// slots > 0 (ww_stream_feed_all; `set` given): every segment is run by `slots` workgroups, one per member slot - the segment table is
// the physical streams', d_state / d_zring / d_zpos are the virtual streams', d_z and d_post hold `slots` planes of plane_rows rows
// and the tail's tables name virtual streams and rows of those planes (launch_plan.h: feed_plan_all).  d_post_rows receives the
// posteriors as [plane_rows][slots].
int ww_k_wave_feed(ww_ctx *ctx, const ww_model *m, const float *d_rows, const wv_feed_seg *d_segs, int n_small, int n_segs,
                   const wv_feed_pool *d_pool, int n_pool, const wv_feed_pool *d_ring, int n_ring, float *d_z, float *d_state,
                   float *d_zring, int32_t *d_zpos, int pidx, float *d_post, const ww_set_ref *set, int slots,
                   int64_t plane_rows, float *d_post_rows) {
  if (n_segs <= 0) return WW_OK;
  if (int rc = ww_wave_seq_check(ctx, m, "ww_stream_feed")) return rc;
  if (slots && (!set || slots > 65535 || plane_rows <= 0 || !d_post_rows)) return ww_fail(ctx, WW_EINTERNAL, "ww_k_wave_feed: %d member slots", slots);
  wave_args a;
  if (int rc = wave_model_args(ctx, m->wave, d_rows, a)) return rc;
  a.tag = {nullptr, 0, pidx};
  wave_seq_args q = {};
  q.state = d_state; q.zring = d_zring; q.zpos = d_zpos; q.P = m->wave.T; q.post = d_post;
  if (slots) a.wa.mel_rows = plane_rows;  // (the rows of a plane of d_z / d_post)
  if (n_small > 0) {
    q.fsegs = d_segs;
    ww_launch_scope scope(ctx, "wavenet_seq_kernel<feed,1>");
    if (slots) hipLaunchKernelGGL((wavenet_seq_kernel<1, false, true, true, true>), dim3(n_small, slots), dim3(64), 0, ctx->stream, a, q, *set);
    else if (set) hipLaunchKernelGGL((wavenet_seq_kernel<1, false, true, true>), dim3(n_small), dim3(64), 0, ctx->stream, a, q, *set);
    else hipLaunchKernelGGL((wavenet_seq_kernel<1, false, true>), dim3(n_small), dim3(64), 0, ctx->stream, a, q, ww_set_ref{});
    WW_HIP(ctx, hipGetLastError());
  }
  if (n_segs > n_small) {
    q.fsegs = d_segs + n_small;
    q.logits = d_z;
    {
      ww_launch_scope scope(ctx, "wavenet_seq_kernel<feed,12>");
      if (slots) hipLaunchKernelGGL((wavenet_seq_kernel<12, false, true, true, true>), dim3(n_segs - n_small, slots), dim3(12 * 64), 0, ctx->stream, a, q, *set);
      else if (set) hipLaunchKernelGGL((wavenet_seq_kernel<12, false, true, true>), dim3(n_segs - n_small), dim3(12 * 64), 0, ctx->stream, a, q, *set);
      else hipLaunchKernelGGL((wavenet_seq_kernel<12, false, true>), dim3(n_segs - n_small), dim3(12 * 64), 0, ctx->stream, a, q, ww_set_ref{});
      WW_HIP(ctx, hipGetLastError());
    }
    ww_launch_scope scope(ctx, "wave_feed_pool_kernels");
    const size_t sm = (size_t)(WW_FEED_POOL_ROWS + q.P - 1) * 16 * sizeof(float);
    if (sm > 64 * 1024) return ww_fail(ctx, WW_EINVAL, "ww_stream_feed: a window of %d rows is beyond the pool kernel's tile", q.P);
    hipLaunchKernelGGL(wave_feed_pool_kernel, dim3(n_pool), dim3(256), sm, ctx->stream, (const float *)d_z, d_pool, a.NOUT, q.P, pidx,
                       (const float *)d_zring, (const int32_t *)d_zpos, d_post);
    hipLaunchKernelGGL(wave_feed_ring_kernel, dim3(n_ring), dim3(256), 0, ctx->stream, (const float *)d_z, d_ring, a.NOUT, q.P, d_zring, d_zpos);
    WW_HIP(ctx, hipGetLastError());
  }
  if (slots) {
    ww_launch_scope scope(ctx, "wave_feed_post_rows_kernel");
    hipLaunchKernelGGL(wave_feed_post_rows_kernel, dim3((unsigned)((plane_rows * slots + 255) / 256)), dim3(256), 0, ctx->stream, (const float *)d_post,
                       plane_rows, slots, d_post_rows);
    WW_HIP(ctx, hipGetLastError());
  }
  return WW_OK;
}

// Which banks take the one-launch tick: those whose ticks stay within the twelve-wave form's range (2 S windows <= 256: one
// workgroup per CU).  Larger banks keep the front-end kernel + the model kernel in its four-wave x three-tile form, which is worth
// more than the launch it costs (tools/stream_forms.py, split-bf16 p50: 128 streams 49.3 vs 54.5 us, 192: 84.9 vs 82.6, 512: 158.7 vs
// 149.2, 1,024: 306.2 vs 273.1; fp32 alike)
bool ww_wave_tick_capable(const ww_model *m, int S) {
  return m->kind == WW_KIND_WAVENET && m->filt.n_mel == 40 && m->wave.n_mel == 40 && m->wave.T + 10 <= WV_T && 2 * S <= wave_wide_from(m);
}

// ONE launch per tick (wavenet_kernel<..., TICK>): 2 S workgroups of twelve waves, the posteriors as tags only
int ww_k_wave_tick(ww_ctx *ctx, const ww_model *m, const ww_tick_fe &fe, int precise, const ww_tick_tag &tag, const ww_set_ref *set) {
  const ww_wave_dev &v = m->wave;
  const ww_filter_dev &f = m->filt;
  if (f.n_mel != 40 || v.n_mel != 40 || fe.hop != 160 || v.T + 10 > WV_T)
    return ww_fail(ctx, WW_EINVAL, "one-launch streaming tick: 40 mel bands, hop 160 and a window of at most %d rows only", WV_T - 10);
  if (!tag.slots || fe.S <= 0) return ww_fail(ctx, WW_EINVAL, "one-launch streaming tick: no tag slots / no streams");
  wave_args a;
  if (int rc = wave_model_args(ctx, v, fe.hist, a)) return rc;
  a.wa = {nullptr, nullptr, 0, 0, 0, (int64_t)fe.S * fe.HR};
  a.tag = tag;
  a.fe = fe;
  a.fb = ww_fe_filt_of(f);
  ww_launch_scope scope(ctx, m->precision == WW_PRECISION_BF16X3 ? "wavenet_kernel<bf16x3,tick>" : "wavenet_kernel<tick>");
  if (precise) wave_launch<2>(ctx, m, 2 * fe.S, a, set);
  else wave_launch<1>(ctx, m, 2 * fe.S, a, set);
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

int ww_k_wave_detect(ww_ctx *ctx, const ww_model *m, const float *d_enc, int nw, float *d_out) {
  if (nw <= 0) return WW_OK;
  wave_args a = wave_head_args(m->wave);
  a.out = d_out; a.enc_in = d_enc;
  ww_launch_scope scope(ctx, "wavenet_detect_kernel");
  hipLaunchKernelGGL((wavenet_kernel<true, false, 12>), dim3(nw), dim3(12 * 64), 0, ctx->stream, a, ww_set_ref{});
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}
