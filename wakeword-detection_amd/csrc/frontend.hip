// PCM -> log-mel front end for gfx950.
//
// Replaces the reference's per-sample RingBuffer loop, np.fft.rfft and the filter.tflite
// invoke (utils/tf_lite/filter.py:38-75; spokestack/wakeword/tflite.py:148-191).
//
// Kernel shape (logmel_kernel, the fp32-FFT profile; the default fp64 front end is logmel_rows_kernel below): one
// 256-thread workgroup (4 wavefronts) stages the samples of FPB = 16 consecutive frames of
// one utterance: the 512 + 15*160 samples those frames touch are loaded ONCE with aligned 16-byte loads
// (straight-line: every load of the block is in flight before the first wait), normalised / clipped /
// pre-emphasised in registers and parked in LDS as fp32.  After that barrier and one more behind the
// Hann products the four wavefronts never meet again; each carries 4 frames to the output, 16 lanes per frame and 16 points per lane: Hann product,
// a radix-16 DFT in registers, twiddles, one 16x16 transpose through LDS (real parts, then
// imaginary parts, same buffer), a second radix-16 DFT - the 256-point complex FFT of the even/odd-packed
// frame - and the real-FFT untangling, for which lane j fetches its partner Z[256-k] (lane (16-j)%16) through
// the dead transpose buffer; two magnitudes per evaluation land in LDS.  The mel filter runs on the vector ALU
// with the lanes re-dealt as (band slot, frame): 64 fused multiply-adds per lane on magnitudes read 16 bytes
// at a time (bands dealt so that these reads are bank-conflict-free: pack_filter in model_pack.h), then the
// log/affine tail, and the wave's 4x40 tile leaves through LDS as one contiguous store.  Wave 3 uses the sample
// tile as its transpose buffer: the tile is dead once every wave has formed its Hann products (the second barrier).
// (This kernel's fp64 form, the default front end of rounds 1-3, is recorded in profiles/EXPERIMENTS.md.)
// logmel_kernel and logmel_rows_kernel are built from one set of pieces, defined once in front of them: LM_STAGE_GENERIC,
// pcm_quot_clip2 and LM_STAGE_SIMPLE_LOAD / LM_STAGE_SIMPLE_STORE (staging), hann_pair, hann_mul_pair and hann_mul_at (Hann
// product), LM_PARTNERS, LM_UNTANGLE_K2 and untangle_tail (real-FFT untangling), LM_MEL_REQ_* and LM_MEL_COMPUTE (the table
// fetches of the mel filter; the filter and the park of the output tile); logmel_lds is logmel_kernel's LDS layout,
// logmel_instance the host's choice of instantiation.
// (stft_mag_kernel and the streaming kernel keep the earlier one-wave-per-frame radix-4 Stockham
// FFT of fft_device.h: they are not on the batched path.)
//
// R = double reproduces the reference numerics (Hann product and FFT in float64,
// spokestack/wakeword/tflite.py:175-176, result cast to float32); R = float is the fast mode.
#include "common.h"

#include "fft_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#ifndef FPB
#define FPB 16  // frames per block
#endif
#define WAVES 4
static_assert(FPB == WAVES * 4, "each wave transforms exactly one group of 4 frames (mags overlay the transposes)");

struct logmel_args {
  const int16_t *pcm;
  const float *f32;
  const int64_t *sample_offs;
  const int64_t *frame_offs;
  int n_utt;
  int tiles_per_utt;  // ceil(longest utterance's frames / FPB)
  int hop;
  float divisor;
  float rdiv;       // RN(1 / divisor)
  int fast_div;     // divisor is 32767 or 32768: 3-op exact quotient (see pcm_quot)
  int clip;
  float preemph;
  // filter
  const int *start;
  const float *wpad;  // [WW_MEL_TAPS][64] tap-major, zero padded
  const float *bias;
  int n_mel;
  float floor_v, log_off, scale;
  const double *hann, *tw256, *tw512, *tw16;
  const float *melV;           // mel filter in lane form: [WW_MELV_CHUNKS][16 slots] float4 (model_pack.h, pack_filter)
  const int *melVmeta;         // [3 groups][16 slots]: first bin | band << 16
  int melv_aligned;            // first bins are multiples of 4: 16-byte magnitude reads
  float *mel;
  // stft-only mode
  const float *frames;
  float *mag_out;
  int64_t n_frames_direct;
  // logmel_rows_kernel: mel rows are numbered through the whole launch
  int64_t total_frames;
  int uniform_nf;      // > 0: every clip has this many frames and uniform_ns samples, clip u starts at sample u * uniform_ns
  int64_t uniform_ns;
  unsigned uni_magic;  // uniform_nf >= 4: row / uniform_nf = __umulhi(row, uni_magic) >> uni_shift for every row < 2^31
  int uni_shift;
};

// int16 / divisor, correctly rounded (reference: frame.astype(np.float32) / 32767, tflite.py:150).
// For the two divisors in use (32767, 32768) the quotient of ANY int16 is obtained exactly by
// q0 = a*r, e = fma(-b, q0, a), q = fma(e, r, q0) with r = RN(1/b) (Markstein); verified
// exhaustively over all 65536 inputs with exact rational arithmetic (tests/test_host_logic.py).
__device__ __forceinline__ float pcm_quot(float x, const logmel_args &a) {
  if (a.fast_div) {
    const float q0 = __fmul_rn(x, a.rdiv);
    const float e = __fmaf_rn(-a.divisor, q0, x);
    return __fmaf_rn(e, a.rdiv, q0);
  }
  return __fdiv_rn(x, a.divisor);
}

template <bool F32IN>
__device__ __forceinline__ float norm_sample(const logmel_args &a, int64_t g) {
  if (F32IN) return a.f32[g];
  float v = pcm_quot((float)a.pcm[g], a);
  if (a.clip) v = fminf(fmaxf(v, -1.0f), 1.0f);
  return v;
}

// ---- radix-16 DFT in registers ------------------------------------------------------------
template <typename R>
__device__ __forceinline__ void radix4(cplx<R> &a0, cplx<R> &a1, cplx<R> &a2, cplx<R> &a3) {
  const cplx<R> t0 = {a0.re + a2.re, a0.im + a2.im}, t1 = {a0.re - a2.re, a0.im - a2.im};
  const cplx<R> t2 = {a1.re + a3.re, a1.im + a3.im}, t3 = {a1.im - a3.im, -(a1.re - a3.re)};  // (a1-a3)*(-i)
  a0 = {t0.re + t2.re, t0.im + t2.im};
  a1 = {t1.re + t3.re, t1.im + t3.im};
  a2 = {t0.re - t2.re, t0.im - t2.im};
  a3 = {t1.re - t3.re, t1.im - t3.im};
}

template <typename R>
__device__ __forceinline__ cplx<R> mulc(cplx<R> a, R wr, R wi) {
  return {a.re * wr - a.im * wi, a.re * wi + a.im * wr};
}

// Forward 16-point DFT, in place.  Input a[n]; output A[k] is left at position 4*(k%4) + k/4.
template <typename R>
__device__ __forceinline__ void dft16(cplx<R> (&a)[16]) {
  constexpr R C = (R)0.92387953251128675613, S = (R)0.38268343236508977173, H = (R)0.70710678118654752440;
#pragma unroll
  for (int q = 0; q < 4; ++q) radix4(a[q], a[q + 4], a[q + 8], a[q + 12]);
  // a[q + 4p] *= W16^(q p),  W16^m = (cos(2 pi m/16), -sin(2 pi m/16))
  a[5] = mulc(a[5], C, -S);   a[9] = mulc(a[9], H, -H);                        a[13] = mulc(a[13], S, -C);
  a[6] = mulc(a[6], H, -H);   a[10] = cplx<R>{a[10].im, -a[10].re};            a[14] = mulc(a[14], -H, -H);
  a[7] = mulc(a[7], S, -C);   a[11] = mulc(a[11], -H, -H);                     a[15] = mulc(a[15], -C, S);
#pragma unroll
  for (int p = 0; p < 4; ++p) radix4(a[4 * p], a[4 * p + 1], a[4 * p + 2], a[4 * p + 3]);
}

__host__ __device__ constexpr int k_of(int pos) { return (pos >> 2) + 4 * (pos & 3); }
__host__ __device__ constexpr int pos_of(int k) { return 4 * (k & 3) + (k >> 2); }


// One wave's LDS instructions are executed in issue order, so a write followed by another
// lane's read (or a read followed by an overwrite) needs no s_waitcnt - only a scheduling fence.
__device__ __forceinline__ void lds_fence() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Sixteen consecutive 8-byte LDS reads as sixteen ds_read_b64 (2 LDS cycles each).  Left to itself the
// compiler pairs them into ds_read2_b64, which the LDS services at 8 cycles per instruction - twice the
// time for the same bytes (MI355X_MICROARCH.md, LDS table).  The reads are issued back to back; the
// caller must lds_wait_all() the destinations before using them.
__device__ __forceinline__ void lds_read16_b64(const double *p, double (&d)[16]) {
  const unsigned a = (unsigned)(uintptr_t)p;  // low 32 bits of a flat LDS pointer = the LDS byte address
#define WW_RD(i) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(d[i]) : "v"(a), "n"((i) * 8))
  WW_RD(0); WW_RD(1); WW_RD(2); WW_RD(3); WW_RD(4); WW_RD(5); WW_RD(6); WW_RD(7);
  WW_RD(8); WW_RD(9); WW_RD(10); WW_RD(11); WW_RD(12); WW_RD(13); WW_RD(14); WW_RD(15);
#undef WW_RD
}
// The same with a stride of 128 bytes: lane j's sample pairs (x[32 n1 + 2j], x[32 n1 + 2j + 1]), n1 = 0..15.
__device__ __forceinline__ void lds_read16_b64_s128(const float *p, double (&d)[16]) {
  const unsigned a = (unsigned)(uintptr_t)p;
#define WW_RD(i) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(d[i]) : "v"(a), "n"((i) * 128))
  WW_RD(0); WW_RD(1); WW_RD(2); WW_RD(3); WW_RD(4); WW_RD(5); WW_RD(6); WW_RD(7);
  WW_RD(8); WW_RD(9); WW_RD(10); WW_RD(11); WW_RD(12); WW_RD(13); WW_RD(14); WW_RD(15);
#undef WW_RD
}
__device__ __forceinline__ void lds_wait_all(double (&d)[16]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4]), "+v"(d[5]), "+v"(d[6]), "+v"(d[7]), "+v"(d[8]),
                 "+v"(d[9]), "+v"(d[10]), "+v"(d[11]), "+v"(d[12]), "+v"(d[13]), "+v"(d[14]), "+v"(d[15])
               :
               : "memory");
}

// An LDS pointer the compiler knows nothing about: constant element offsets from it then travel in the
// instruction's offset field instead of costing one vector add per access.
typedef __attribute__((address_space(3))) const float lds_cfloat;
typedef __attribute__((address_space(3))) const f32x4 lds_cfloat4;
__device__ __forceinline__ lds_cfloat *lds_opaque(const float *p) {
  unsigned a = (unsigned)(uintptr_t)p;  // low 32 bits of a flat LDS pointer = the LDS byte address
  asm volatile("" : "+v"(a));
  return (lds_cfloat *)(uintptr_t)a;
}

// (h[2n], h[2n+1]) for n = 16 n1 + j from the half table of 128 pairs (h[m] = h[511 - m])
template <typename H2>
__device__ __forceinline__ H2 hann_pair(const H2 *tb, int n1, int j) {
  if (n1 < 8) return tb[16 * n1 + j];
  const H2 m = tb[16 * (15 - n1) + 15 - j];
  H2 r;
  r.x = m.y;
  r.y = m.x;
  return r;
}

// MAG_LD (model_layout.h) = 272 floats per frame of magnitudes: 257 + zero pad to 17*16; 16 mod 32, so the two frames a
// 32-lane write group touches use disjoint banks
#define TR_LD 17    // padded row of the 16x16 transpose
#define LM_WBUF (4 * MAG_LD * 4)  // logmel_kernel's per-wave scratch: 16x16 fp32 transposes of 4 frames, later their magnitudes

// ---- pieces shared by logmel_kernel (256 threads on a 16-frame tile) and logmel_rows_kernel (one wave on four frames) ---------
// Functions where both kernels keep their instruction stream, single-statement macros where a function moved it
// (profiles/EXPERIMENTS.md, section 16); a macro's own names end in an underscore, thread index and stride are arguments.

// Generic staging: dst[q * VEC + e] = normalised (and pre-emphasised) sample ga + q * VEC + e for q < n_vec, dealt to STRIDE
// threads; ga is a multiple of VEC, so every full vector is one aligned 16-byte load
#define LM_STAGE_GENERIC(F32IN_, STRIDE_, a_, dst_, ga_, n_vec_, s_begin_, total_, tid_)                                   \
  do {                                                                                                                 \
    constexpr int VEC_ = (F32IN_) ? 4 : 8;                                                                             \
    const float alpha_ = (a_).preemph;                                                                                 \
    for (int q_ = (tid_); q_ < (n_vec_); q_ += (STRIDE_)) {                                                            \
      const int64_t g_ = (ga_) + (int64_t)q_ * VEC_;                                                                   \
      float v_[VEC_ + 1];                                                                                              \
      /* v_[0] = sample g-1 (pre-emphasis carry; 0 at the start of the utterance) */                                   \
      v_[0] = (alpha_ != 0.0f && g_ - 1 >= (s_begin_)) ? norm_sample<F32IN_>(a_, g_ - 1) : 0.0f;                       \
      if (g_ + VEC_ <= (total_)) {                                                                                     \
        if (F32IN_) {                                                                                                  \
          const float4 raw_ = *(const float4 *)((a_).f32 + g_);                                                        \
          v_[1] = raw_.x; v_[2] = raw_.y; v_[3] = raw_.z; v_[4] = raw_.w;                                              \
        } else {                                                                                                       \
          const uint4 raw_ = *(const uint4 *)((a_).pcm + g_);                                                          \
          const unsigned int w32_[4] = {raw_.x, raw_.y, raw_.z, raw_.w};                                               \
          _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) {                                                           \
            const int16_t s16_ = (int16_t)((w32_[e_ >> 1] >> ((e_ & 1) * 16)) & 0xffffu);                              \
            float f_ = pcm_quot((float)s16_, a_);                                                                      \
            if ((a_).clip) f_ = fminf(fmaxf(f_, -1.0f), 1.0f);                                                         \
            v_[1 + e_] = f_;                                                                                           \
          }                                                                                                            \
        }                                                                                                              \
      } else { /* ragged end of the whole buffer */                                                                    \
        _Pragma("unroll") for (int e_ = 0; e_ < VEC_; ++e_)                                                            \
          v_[1 + e_] = (g_ + e_ < (total_)) ? norm_sample<F32IN_>(a_, g_ + e_) : 0.0f;                                 \
      }                                                                                                                \
      float o_[VEC_];                                                                                                  \
      _Pragma("unroll") for (int e_ = 0; e_ < VEC_; ++e_) {                                                            \
        /* reference: frame -= pre_emphasis * previous  (separate fp32 multiply and subtract).  Slots in front of the  \
           utterance start are never read by a frame of this utterance, except that sample s_begin itself must see a   \
           zero carry (v_[0] above / guard here). */                                                                   \
        const float prev_ = (g_ + e_ == (s_begin_)) ? 0.0f : v_[e_];                                                   \
        o_[e_] = (alpha_ != 0.0f) ? ww_preemph_rn(v_[1 + e_], alpha_, prev_) : v_[1 + e_];                             \
      }                                                                                                                \
      float4 *d4_ = (float4 *)((dst_) + (size_t)q_ * VEC_);                                                            \
      d4_[0] = make_float4(o_[0], o_[1], o_[2], o_[3]);                                                                \
      if (VEC_ == 8) d4_[1] = make_float4(o_[4], o_[5], o_[6], o_[7]);                                                 \
    }                                                                                                                  \
  } while (0)
// logmel_rows_kernel stages from two places: one wave's instance of the above
template <bool F32IN>
__device__ __forceinline__ void stage_generic_wave(const logmel_args &a, float *dst, int64_t ga, int n_vec, int64_t s_begin,
                                                   int64_t total, int lane) {
  LM_STAGE_GENERIC(F32IN, 64, a, dst, ga, n_vec, s_begin, total, lane);
}

// The exact quotient (see pcm_quot) and the clip on the two int16 samples of one 32-bit word: v_pk_mul_f32 / v_pk_fma_f32, two
// samples per issue; lim = 1 or +inf
__device__ __forceinline__ void pcm_quot_clip2(const logmel_args &a, unsigned int w32, float lim, float &o0, float &o1) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 r2 = {a.rdiv, a.rdiv}, nb2 = {-a.divisor, -a.divisor};
  const f32x2 x = {(float)(int)(short)(w32 & 0xffffu), (float)((int)w32 >> 16)};
  const f32x2 q0 = x * r2;
  const f32x2 er = __builtin_elementwise_fma(nb2, q0, x);
  const f32x2 q = __builtin_elementwise_fma(er, r2, q0);
  o0 = __builtin_amdgcn_fmed3f(q.x, -lim, lim);
  o1 = __builtin_amdgcn_fmed3f(q.y, -lim, lim);
}

// Straight-line staging (no pre-emphasis, divisor 32767/32768: the host checks), NV 16-byte vectors per thread of STRIDE threads,
// indices of type idx_t: LM_STAGE_SIMPLE_LOAD requests all NV vectors before anything waits for one - the caller may put loads of
// its own behind them - and LM_STAGE_SIMPLE_STORE normalises / clips them into tile[q * VEC ..], q = tid + STRIDE h < n_vec.
// A load index is clamped: always a full vector inside the buffer, and never past this tile's last vector (threads beyond
// it would otherwise pull the NEXT tile's lines through this XCD's L2: +40 % fabric traffic).
#define LM_STAGE_SIMPLE_LOAD(F32IN_, NV_, STRIDE_, idx_t_, a_, ga_, n_vec_, total_, tid_, gq_, raw_)                        \
  do {                                                                                                                 \
    constexpr int VEC_ = (F32IN_) ? 4 : 8;                                                                             \
    const idx_t_ last_ = ((total_) - VEC_) & ~(idx_t_)(VEC_ - 1); /* last full aligned vector (total >= WIN here) */   \
    const idx_t_ tile_last_ = (ga_) + (idx_t_)((n_vec_) - 1) * VEC_;                                                   \
    _Pragma("unroll") for (int h_ = 0; h_ < (NV_); ++h_) {                                                             \
      (gq_)[h_] = (ga_) + (idx_t_)((tid_) + (STRIDE_) * h_) * VEC_;                                                    \
      idx_t_ gl_ = (gq_)[h_] < tile_last_ ? (gq_)[h_] : tile_last_;                                                    \
      gl_ = gl_ < last_ ? gl_ : last_;                                                                                 \
      (raw_)[h_] = (F32IN_) ? *(const uint4 *)((a_).f32 + gl_) : *(const uint4 *)((a_).pcm + gl_);                     \
    }                                                                                                                  \
  } while (0)
#define LM_STAGE_SIMPLE_STORE(F32IN_, NV_, STRIDE_, idx_t_, a_, tile_, n_vec_, total_, tid_, gq_, raw_)                     \
  do {                                                                                                                 \
    constexpr int VEC_ = (F32IN_) ? 4 : 8;                                                                             \
    const idx_t_ last_ = ((total_) - VEC_) & ~(idx_t_)(VEC_ - 1);                                                      \
    const float lim_ = (a_).clip ? 1.0f : __builtin_inff();                                                            \
    _Pragma("unroll") for (int h_ = 0; h_ < (NV_); ++h_) {                                                             \
      const int q_ = (tid_) + (STRIDE_) * h_;                                                                          \
      if (q_ < (n_vec_)) {                                                                                             \
        float o_[VEC_];                                                                                                \
        if ((gq_)[h_] <= last_) {                                                                                      \
          const unsigned int w32_[4] = {(raw_)[h_].x, (raw_)[h_].y, (raw_)[h_].z, (raw_)[h_].w};                       \
          if (F32IN_) {                                                                                                \
            _Pragma("unroll") for (int e_ = 0; e_ < VEC_; ++e_) o_[e_] = __uint_as_float(w32_[e_]);                    \
          } else {                                                                                                     \
            _Pragma("unroll") for (int e_ = 0; e_ < VEC_; e_ += 2) pcm_quot_clip2(a_, w32_[e_ >> 1], lim_, o_[e_], o_[e_ + 1]); \
          }                                                                                                            \
        } else { /* ragged end of the whole buffer: element-wise, zero beyond it */                                    \
          _Pragma("unroll") for (int e_ = 0; e_ < VEC_; ++e_)                                                          \
            o_[e_] = ((gq_)[h_] + e_ < (total_)) ? norm_sample<F32IN_>(a_, (int64_t)(gq_)[h_] + e_) : 0.0f;            \
        }                                                                                                              \
        float4 *d4_ = (float4 *)((tile_) + (size_t)q_ * VEC_);                                                         \
        d4_[0] = make_float4(o_[0], o_[1], o_[2], o_[3]);                                                              \
        if (VEC_ == 8) d4_[1] = make_float4(o_[4], o_[5], o_[6], o_[7]);                                               \
      }                                                                                                                \
    }                                                                                                                  \
  } while (0)

// Hann product of one n1 (pass 1: lane j holds z[16 n1 + j] = (x[2n] h[2n], x[2n+1] h[2n+1]), n = 16 n1 + j) from the sample pair
// an 8-byte LDS read delivered, and from two scalar reads (odd shift or hop).  fp32: tflite.py:175 forms the product in fp64.
template <typename R, typename H2>
__device__ __forceinline__ cplx<R> hann_mul_pair(double xs, const H2 h) {
  return {(R)((R)__int_as_float(__double2loint(xs)) * h.x), (R)((R)__int_as_float(__double2hiint(xs)) * h.y)};
}
template <typename R, typename H2>
__device__ __forceinline__ cplx<R> hann_mul_at(const float *src, int n, const H2 h) {
  return {(R)((R)src[2 * n] * h.x), (R)((R)src[2 * n + 1] * h.y)};
}

// Real-FFT untangling.  With a = Z[k], b = conj Z[256-k]:  2E = a+b, 2O = (a-b)/i, 2T = W512^k 2O and
//   2X[k] = 2E + 2T,   2X[256-k] = conj(2E - 2T)   ->  two magnitudes per evaluation, k < 128 only;
//   the factor 2 leaves as an exact 0.5 after the fp32 square root.
// After the second DFT pass lane j register k2 holds k = j + 16 k2; its partner Z[256-k] lives in lane (16-j)%16 at
// k2' = 15-k2 (j > 0) or in the same lane at k2' = (16-k2)%16 (j = 0).  LM_PARTNERS brings the eight partners of k2 = 0..7
// into pz_[8] through the (dead) transpose buffer trs_ of this frame: rows 8..15 <- registers k2' = 8..15, row 7 <- k2' = 0
// (only lane 0 reads that one), so lane j reads row 15-k2 (+1 for j = 0; row 7 for k2 = 0); real parts, then imaginary parts.
#define LM_PARTNERS(R_, w_, trs_, j_, pz_)                                                          \
  do {                                                                                              \
    const int pj_ = (16 - (j_)) & 15;                                                               \
    const R_ *prow0_ = (trs_) + ((j_) == 0 ? 7 : 15) * TR_LD + pj_;                                 \
    const R_ *prow_ = (trs_) + ((j_) == 0 ? 16 : 15) * TR_LD + pj_;                                 \
    (trs_)[7 * TR_LD + (j_)] = (w_)[pos_of(0)].re;                                                  \
    _Pragma("unroll") for (int r_ = 8; r_ < 16; ++r_) (trs_)[r_ * TR_LD + (j_)] = (w_)[pos_of(r_)].re; \
    lds_fence();                                                                                    \
    (pz_)[0].re = prow0_[0];                                                                        \
    _Pragma("unroll") for (int k2_ = 1; k2_ < 8; ++k2_) (pz_)[k2_].re = prow_[-k2_ * TR_LD];        \
    lds_fence();                                                                                    \
    (trs_)[7 * TR_LD + (j_)] = (w_)[pos_of(0)].im;                                                  \
    _Pragma("unroll") for (int r_ = 8; r_ < 16; ++r_) (trs_)[r_ * TR_LD + (j_)] = (w_)[pos_of(r_)].im; \
    lds_fence();                                                                                    \
    (pz_)[0].im = prow0_[0];                                                                        \
    _Pragma("unroll") for (int k2_ = 1; k2_ < 8; ++k2_) (pz_)[k2_].im = prow_[-k2_ * TR_LD];        \
    lds_fence();                                                                                    \
  } while (0)

// One k = j + 16 k2 < 128 from own = Z[k], its partner p = Z[256 - k] and un = W512^k: magnitudes 2|X[k]| and 2|X[256 - k]|
// into the frame's row (the mel weights carry the 0.5)
#define LM_UNTANGLE_K2(R_, own_, p_, un_, mrow_, k_)                                                        \
  do {                                                                                                   \
    const cplx<R_> o_ = (own_), u_ = (un_);                                                              \
    const R_ er_ = o_.re + (p_).re, ei_ = o_.im - (p_).im;                                               \
    const R_ or_ = o_.im + (p_).im, oi_ = (p_).re - o_.re;                                               \
    const R_ tr_ = or_ * u_.re - oi_ * u_.im, ti_ = or_ * u_.im + oi_ * u_.re;                           \
    const R_ pr_ = er_ + tr_, pi_ = ei_ + ti_, qr_ = er_ - tr_, qi_ = ei_ - ti_;                         \
    (mrow_)[(k_)] = __builtin_amdgcn_sqrtf((float)(pr_ * pr_ + pi_ * pi_));                              \
    (mrow_)[256 - (k_)] = __builtin_amdgcn_sqrtf((float)(qr_ * qr_ + qi_ * qi_)); /* k = 0 -> bin 256 */ \
  } while (0)
// k = 128 pairs with itself: X[128] = conj(Z[128]) (lane 0, k2 = 8: z); bins 257..271 are zero padding
template <typename R>
__device__ __forceinline__ void untangle_tail(const cplx<R> z, float *mrow, int j) {
  if (j == 0) mrow[128] = 2.0f * __builtin_amdgcn_sqrtf((float)(z.re * z.re + z.im * z.im));
  else mrow[256 + j] = 0.0f;
}

// Mel filterbank on the vector ALU, per wave, on the wave's four rows of magnitudes mg_[4][MAG_LD], and the park of its
// 4 x n_mel tile at mg_ for one contiguous store.  Lane 4 s + q owns frame q and slot s of each of the three
//   band groups (pack_filter, model_pack.h): 36 + 16 + 12 padded taps, one fused multiply-add per tap with the
//   magnitudes read 16 bytes at a time from this wave's LDS rows.  Frame in the low lane bits: the four
//   16-lane groups a ds_read_b128 is served in then hold four slots x four frames each, the rows of the four
//   frames sit 4 sixteen-byte bank slots apart, and pack_filter deals the bands so that the four slots of such
//   a group start on different slots mod 4 - conflict-free.  (The fp32 MFMA form of this contraction kept
//   the SIMD's vector ALU idle for 32 cycles per instruction - fp32 MFMA and VALU share a datapath on gfx950
//   - and needed three workgroup barriers for the partial sums; this form needs none.)
// The tail comes in two halves.  What the request half fetches - a lane's three meta words, its three biases (addressed by
// meta) and the weight chunks of its slot - depends on (lane_ >> 2) and the model alone, on nothing the wave computes, so a
// kernel may ask for it as early as it has registers to receive it: LM_MEL_REQ_META, LM_MEL_REQ_BIAS (waits for meta) and
// LM_MEL_REQ_W per group, in that order.  Registers are the one constraint: the weights must not be live across the FFT, whose
// data fills the file, and while group 0 runs its 36 weights sit beside its 36 magnitudes, which leaves room for the 16 of
// group 1 in a 104-register wave and for neither group 1's nor the 12 of group 2 in a 92-register one.  So the caller
// requests the groups below ahead_ and the compute half the others: group 0, if it is among them, where its turn comes, the
// rest behind group 0's FMAs, where they have the log tail of group 0 and the whole of group 1 to arrive in.  The compute half reads q_ from registers, group 0 first: loads return in
// order, so each group waits with a counted vmcnt for its own chunks only.  Without melv_aligned the magnitudes are read a
// float at a time.  Empty slots write to a spare word each so that the code stays straight-line.
struct lm_mel_fetch {
  int meta[WW_MELV_GROUPS];  // first bin | band << 16 of this lane's slot in each group
  float bias[WW_MELV_GROUPS];
  float4 wq[WW_MELV_CHUNKS];
};
#define LM_MEL_LOGTAIL(a_, acc_, bias_) ((logf(fmaxf((acc_) + (bias_), (a_).floor_v)) + (a_).log_off) * (a_).scale)
#define LM_MEL_REQ_META(a_, lane_, q_)                                                                                 \
  do {                                                                                                                 \
    const unsigned j_ = (unsigned)(lane_) >> 2; /* slot of this lane */                                                \
    _Pragma("unroll") for (int g_ = 0; g_ < WW_MELV_GROUPS; ++g_) (q_).meta[g_] = (a_).melVmeta[g_ * 16 + j_];         \
  } while (0)
#define LM_MEL_REQ_BIAS(a_, q_)                                                                                        \
  do {                                                                                                                 \
    _Pragma("unroll") for (int g_ = 0; g_ < WW_MELV_GROUPS; ++g_) {                                                    \
      const int band_ = (int)((unsigned)(q_).meta[g_] >> 16); /* 0xffff: empty slot */                                 \
      (q_).bias[g_] = (a_).bias[band_ < (a_).n_mel ? band_ : 0];                                                       \
    }                                                                                                                  \
  } while (0)
#define LM_MEL_REQ_W(a_, lane_, q_, g_)                                                                                \
  do {                                                                                                                 \
    constexpr int RCAPQ_[WW_MELV_GROUPS] = WW_MELV_CAPQ, RC0_[WW_MELV_GROUPS] = WW_MELV_CHUNK0;                        \
    const float4 *wv_ = (const float4 *)(a_).melV + ((unsigned)(lane_) >> 2);                                          \
    _Pragma("unroll") for (int c_ = 0; c_ < RCAPQ_[g_]; ++c_) (q_).wq[RC0_[g_] + c_] = wv_[(RC0_[g_] + c_) * 16];      \
  } while (0)
#define LM_MEL_REQ_REST(a_, lane_, q_, g_, ahead_)                                                                     \
  do {                                                                                                                 \
    if ((g_) == 0 && (ahead_) < WW_MELV_GROUPS) {                                                                      \
      __builtin_amdgcn_sched_barrier(0);                                                                               \
      _Pragma("unroll") for (int h_ = (ahead_) > 1 ? (ahead_) : 1; h_ < WW_MELV_GROUPS; ++h_)                          \
        LM_MEL_REQ_W(a_, lane_, q_, h_);                                                                               \
      __builtin_amdgcn_sched_barrier(0);                                                                               \
    }                                                                                                                  \
  } while (0)
#define LM_MEL_COMPUTE(a_, mg_, lane_, q_, ahead_)                                                                     \
  do {                                                                                                                 \
    const int sub_ = (lane_) & 3; /* frame of this lane (its slot: lane_ >> 2) */                                      \
    constexpr int CAPQ_[WW_MELV_GROUPS] = WW_MELV_CAPQ, C0_[WW_MELV_GROUPS] = WW_MELV_CHUNK0;                          \
    const float *mrow_ = (mg_) + sub_ * MAG_LD;                                                                        \
    float res_[3];                                                                                                     \
    if ((a_).melv_aligned) {                                                                                           \
      _Pragma("unroll") for (int g_ = 0; g_ < 3; ++g_) {                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        if (g_ == 0 && (ahead_) == 0) LM_MEL_REQ_W(a_, lane_, q_, 0);                                                  \
        lds_cfloat4 *mb_ = (lds_cfloat4 *)lds_opaque(mrow_ + ((q_).meta[g_] & 0xffff));                                \
        float acc_ = 0.f, acc1_ = 0.f; /* two chains: a dependent fp32 FMA does not issue back to back */              \
        _Pragma("unroll") for (int c_ = 0; c_ < CAPQ_[g_]; ++c_) {                                                     \
          const float4 w4_ = (q_).wq[C0_[g_] + c_];                                                                    \
          const f32x4 m4_ = mb_[c_];                                                                                   \
          acc_ = fmaf(m4_[0], w4_.x, acc_);                                                                            \
          acc1_ = fmaf(m4_[1], w4_.y, acc1_);                                                                          \
          acc_ = fmaf(m4_[2], w4_.z, acc_);                                                                            \
          acc1_ = fmaf(m4_[3], w4_.w, acc1_);                                                                          \
        }                                                                                                              \
        acc_ += acc1_;                                                                                                 \
        LM_MEL_REQ_REST(a_, lane_, q_, g_, ahead_);                                                                    \
        res_[g_] = LM_MEL_LOGTAIL(a_, acc_, (q_).bias[g_]);                                                            \
      }                                                                                                                \
    } else {                                                                                                           \
      _Pragma("unroll") for (int g_ = 0; g_ < 3; ++g_) {                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        if (g_ == 0 && (ahead_) == 0) LM_MEL_REQ_W(a_, lane_, q_, 0);                                                  \
        lds_cfloat *mb_ = lds_opaque(mrow_ + ((q_).meta[g_] & 0xffff));                                                \
        float acc_ = 0.f;                                                                                              \
        _Pragma("unroll") for (int c_ = 0; c_ < CAPQ_[g_]; ++c_) {                                                     \
          const float4 w4_ = (q_).wq[C0_[g_] + c_];                                                                    \
          acc_ = fmaf(mb_[4 * c_ + 0], w4_.x, acc_);                                                                   \
          acc_ = fmaf(mb_[4 * c_ + 1], w4_.y, acc_);                                                                   \
          acc_ = fmaf(mb_[4 * c_ + 2], w4_.z, acc_);                                                                   \
          acc_ = fmaf(mb_[4 * c_ + 3], w4_.w, acc_);                                                                   \
        }                                                                                                              \
        LM_MEL_REQ_REST(a_, lane_, q_, g_, ahead_);                                                                    \
        res_[g_] = LM_MEL_LOGTAIL(a_, acc_, (q_).bias[g_]);                                                            \
      }                                                                                                                \
    }                                                                                                                  \
    lds_fence(); /* the magnitudes are dead */                                                                         \
    _Pragma("unroll") for (int g_ = 0; g_ < 3; ++g_) {                                                                 \
      const int band_ = (int)((unsigned)(q_).meta[g_] >> 16);                                                          \
      (mg_)[band_ < (a_).n_mel ? sub_ * (a_).n_mel + band_ : 4 * (a_).n_mel + (lane_)] = res_[g_];                     \
    }                                                                                                                  \
    lds_fence();                                                                                                       \
  } while (0)

// logmel_kernel's dynamic LDS, byte offsets: what the kernel forms its pointers from and the launcher its size
struct logmel_lds {
  // Hann table: np.hanning is symmetric (h[n] = h[511 - n]), so the first 256 values serve as 128 pairs (float2, in the slots
  // of the fp64 form's double2); twiddle tables [k1][j] = W256^(j k1) and W512^k; one buffer per wave but the last, which uses the
  // sample tile: that is dead once every wave has formed its Hann products (the second barrier)
  static constexpr size_t hann = 0;
  static constexpr size_t tw = hann + 128 * sizeof(double2);
  static constexpr size_t un = tw + 256 * sizeof(cplx<float>);
  static constexpr size_t wbuf = un + 256 * sizeof(cplx<float>);
  static constexpr size_t tile = wbuf + (WAVES - 1) * LM_WBUF;  // fp32 samples, [WIN + (FPB-1)*hop + 16]
  static size_t bytes(int hop) {
    size_t tile_b = (size_t)(WIN + (FPB - 1) * hop + 16) * 4;
    if (tile_b < (size_t)LM_WBUF) tile_b = LM_WBUF;  // the last wave's buffer
    return (tile + tile_b + 15) & ~size_t(15);
  }
};

template <bool F32IN, bool SIMPLE>
__global__ __launch_bounds__(256, 5) void logmel_kernel(logmel_args a) {
  extern __shared__ __align__(16) unsigned char smem[];
  typedef float R;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, sub = lane >> 4;
  // XCD-aware order: workgroup ids go round-robin to the 8 XCDs (id % 8), each with its own L2.  Adjacent
  // tiles of an utterance share 352 of their 2 912 samples, so all tiles of utterance u are given ids of
  // residue u % 8: the shared lines are then fetched once per utterance instead of once per tile.
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int u = (slot / a.tiles_per_utt) * 8 + xcd, tile_idx = slot % a.tiles_per_utt;
  if (u >= a.n_utt) return;
  const int64_t s_begin = a.sample_offs[u], s_end = a.sample_offs[u + 1];
  const int64_t n_samples = s_end - s_begin;
  const int64_t nf = n_samples >= WIN ? (n_samples - WIN) / a.hop + 1 : 0;
  const int64_t f0 = (int64_t)tile_idx * FPB;
  if (f0 >= nf) return;
  const int nfb = (int)((nf - f0) < FPB ? (nf - f0) : FPB);

  // ---- LDS carve-up
  typedef float2 H2;
  H2 *tb_hann = (H2 *)(smem + logmel_lds::hann);
  cplx<R> *tb_tw = (cplx<R> *)(smem + logmel_lds::tw);
  cplx<R> *tb_un = (cplx<R> *)(smem + logmel_lds::un);
  unsigned char *wbuf = smem + logmel_lds::wbuf;
  float *tile = (float *)(smem + logmel_lds::tile);

  // ---- stage the sample tile: aligned 16-byte global loads; tile[i + shift] = x[g_first + i]
  constexpr int VEC = F32IN ? 4 : 8;                      // elements per 16-byte load
  const int64_t g_first = s_begin + f0 * a.hop;           // first sample of frame f0
  const int n_need = WIN + (nfb - 1) * a.hop;             // samples used by this block
  const int shift = (int)(g_first % VEC);
  auto fill_tables = [&](const double2 hv, const double2 twv) {
    if (tid < 128) {
      H2 hq;
      hq.x = hv.x;
      hq.y = hv.y;
      tb_hann[tid] = hq;
    }
    tb_tw[tid] = {(R)twv.x, (R)twv.y};
    tb_un[tid] = {(R)a.tw512[2 * tid], (R)a.tw512[2 * tid + 1]};
  };
  if (SIMPLE) {
    // No pre-emphasis, divisor 32767/32768, at most two 16-byte vectors per thread (host checks):
    // straight-line code - both sample loads and the table load are in flight together, so the
    // block pays one memory latency before its first barrier instead of four in a row.
    const int64_t ga = g_first - shift;                   // multiple of VEC, >= 0
    const int n_vec = (shift + n_need + VEC - 1) / VEC;
    const int64_t total = a.sample_offs[a.n_utt];
    int64_t gq[2];
    uint4 raw[2];
    LM_STAGE_SIMPLE_LOAD(F32IN, 2, 256, int64_t, a, ga, n_vec, total, tid, gq, raw);
    const double2 hv = *(const double2 *)(a.hann + 2 * (tid & 127));
    const double2 twv = *(const double2 *)(a.tw16 + 2 * tid);
    LM_STAGE_SIMPLE_STORE(F32IN, 2, 256, int64_t, a, tile, n_vec, total, tid, gq, raw);
    fill_tables(hv, twv);
  } else {
    fill_tables(*(const double2 *)(a.hann + 2 * (tid & 127)), *(const double2 *)(a.tw16 + 2 * tid));
    const int64_t ga = g_first - shift;                   // multiple of VEC, >= 0
    const int n_vec = (shift + n_need + VEC - 1) / VEC;
    const int64_t total = a.sample_offs[a.n_utt];
    LM_STAGE_GENERIC(F32IN, 256, a, tile, ga, n_vec, s_begin, total, tid);
  }
  __syncthreads();

  // ---- FFT: every 16-lane row of a wave owns one frame (4 frames per wave at a time)
  unsigned char *wb = wave == WAVES - 1 ? (unsigned char *)tile : wbuf + (size_t)wave * LM_WBUF;
  R *tr = (R *)wb;          // [4][16][TR_LD]
  float *mg = (float *)wb;  // overlay: [4][MAG_LD]
  const int fb = wave * 4;
  const bool active = fb < nfb;
  cplx<R> v[16];
  if (active) {
    int f = fb + sub;
    f = f < nfb ? f : nfb - 1;  // surplus rows recompute the last frame (results unused)
    const float *src = tile + shift + f * a.hop;
    // pass 1: lane j holds z[16 n1 + j], n1 = 0..15; Hann product (in fp32: tflite.py:175 forms it in fp64)
    if (((shift | a.hop) & 1) == 0) {  // block-uniform
      // 8-byte aligned pairs: ds_read_b64 (a quarter of the LDS time of the two-dword form, and with hop = 160
      // the four frames of a wave sit 32 banks apart: conflict-free)
      double xs[16];
      lds_read16_b64_s128(src + 2 * j, xs);
      H2 h[16];
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) h[n1] = hann_pair(tb_hann, n1, j);
      lds_wait_all(xs);
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) v[n1] = hann_mul_pair<R>(xs[n1], h[n1]);
    } else {
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) {
        const H2 h = hann_pair(tb_hann, n1, j);
        v[n1] = hann_mul_at<R>(src, 16 * n1 + j, h);
      }
    }
  }
  __syncthreads();  // the sample tile is dead now - wave 3's transposes and magnitudes move in
  // From here on the four waves never meet again: each one carries its own 4 frames to the output.
  if (!active) return;
  lm_mel_fetch mq;
  {
    dft16<R>(v);
#pragma unroll
    for (int pos = 1; pos < 16; ++pos) v[pos] = cmul(v[pos], tb_tw[k_of(pos) * 16 + j]);
    // 16x16 transpose through LDS, real parts then imaginary parts (same buffer)
    cplx<R> w[16];
    R *trs = tr + sub * 16 * TR_LD;
#pragma unroll
    for (int pos = 0; pos < 16; ++pos) trs[k_of(pos) * TR_LD + j] = v[pos].re;
    lds_fence();
#pragma unroll
    for (int n2 = 0; n2 < 16; ++n2) w[n2].re = trs[j * TR_LD + n2];
    lds_fence();
#pragma unroll
    for (int pos = 0; pos < 16; ++pos) trs[k_of(pos) * TR_LD + j] = v[pos].im;
    lds_fence();
#pragma unroll
    for (int n2 = 0; n2 < 16; ++n2) w[n2].im = trs[j * TR_LD + n2];
    lds_fence();
    // pass 2: lane j = k1 holds Y[n2][k1]; output w[pos] = Z[k1 + 16 k_of(pos)]
    dft16<R>(w);
    // the mel tail's meta words and biases arrive under the untangling; its weights (92 registers) are left to LM_MEL_COMPUTE
    __builtin_amdgcn_sched_barrier(0);
    LM_MEL_REQ_META(a, lane, mq);
    __builtin_amdgcn_sched_barrier(0);
    // untangle: the partners Z[256 - k] arrive through the (dead) transpose buffer, W512^k from the LDS table
    cplx<R> pz[8];
    LM_PARTNERS(R, w, trs, j, pz);
    __builtin_amdgcn_sched_barrier(0);
    LM_MEL_REQ_BIAS(a, mq);
    __builtin_amdgcn_sched_barrier(0);
    float *mrow = mg + sub * MAG_LD;
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) LM_UNTANGLE_K2(R, w[pos_of(k2)], pz[k2], tb_un[j + 16 * k2], mrow, j + 16 * k2);
    untangle_tail<R>(w[pos_of(8)], mrow, j);
  }

  // ---- mel filterbank and the park of the wave's 4 x n_mel tile, which leaves as one contiguous store
  lds_fence();
  {
    LM_MEL_COMPUTE(a, mg, lane, mq, 0);
    const int nv = (nfb - fb) < 4 ? (nfb - fb) : 4;
    float *dstf = a.mel + (a.frame_offs[u] + f0 + fb) * (int64_t)a.n_mel;
    if ((((uintptr_t)dstf) & 15) == 0 && (a.n_mel & 3) == 0) {
      for (int i = lane; i < nv * a.n_mel / 4; i += 64) ((float4 *)dstf)[i] = ((const float4 *)mg)[i];
    } else {
      for (int i = lane; i < nv * a.n_mel; i += 64) dstf[i] = mg[i];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// logmel_rows_kernel (round 4): the fp64 front end with next to nothing shared between the waves of a workgroup
// (since section 24 of profiles/EXPERIMENTS.md: the Hann half table, behind one barrier at the top).
//
// Why.  In the pipelined step the front end of batch i+1 runs in the shadow of batch i's crnn_fused_kernel, whose one
// wave per SIMD keeps the shared fp32-MFMA / vector datapath about half busy; how much of the other half the front end
// picks up is set by how many of its waves fit beside a CRNN workgroup.  The fp64 tile kernel of rounds 1-3 cost 10 KB of LDS and
// 128 registers per wave (40 KB per 4-wave workgroup: the 16-frame sample tile + Hann table + three transpose buffers), so two
// workgroups = 8 waves fit.  This kernel costs 8.5 KB and 104 registers per wave and one workgroup barrier, in front of the transform:
//   * a wave owns the four consecutive GLOBAL frames 4 W .. 4 W + 3 of the launch (mel rows are numbered through all
//     clips), so tiles run across clip boundaries: 37,632 frames = 9,408 full waves, none of the 256 three-frame tiles of
//     the per-clip tiling, and ragged batches leave no partly filled workgroups behind;
//   * it stages its own samples (<= 512 + 3 hop, two 16-byte loads per lane) into ITS transpose buffer, which is dead
//     until the first DFT pass is over: LDS instructions of one wave execute in order, so neither the hand-over of the
//     buffer from tile to transposes to magnitudes to the output tile nor the staging needs a barrier;
//   * Hann pairs come from the workgroup's Hann block in LDS (LW_HANN_N below), twiddles from the L1-resident tables (4 + 4 KB,
//     shared by every wave of the chip);
//   * 104 registers (amdgpu_num_vgpr counts in units of two on gfx90a+): the Hann products, the inter-pass twiddles and the
//     untangling twiddles are software-pipelined by hand in chunks of 4 / 3 / 2 instead of all at once, and the mel
//     weights are requested as the untangling retires registers: three of these waves sit on a SIMD beside a 184-register
//     CRNN wave, four alone.
// A wave whose four frames do not lie in one clip within 3 hops of each other (a clip boundary) stages them frame by frame
// (generic path, <= 1 wave in 37 for 1.5 s clips).  The arithmetic is that of the fp64 tile kernel it replaced, instruction for
// instruction, with bit-identical results (profiles/EXPERIMENTS.md, round 4).
// What it has in common with logmel_kernel is the shared pieces above, instantiated for one wave and R = double: staging
// (LM_STAGE_SIMPLE_LOAD / LM_STAGE_SIMPLE_STORE with NV vectors per lane and idx_t indices; stage_generic_wave = LM_STAGE_GENERIC at
// stride 64), lw_hann_pair on the Hann block with hann_mul_pair / hann_mul_at per chunk of LW_HC, LM_PARTNERS,
// LM_UNTANGLE_K2 on a register chunk of W512^k, untangle_tail, LM_MEL_REQ_* and LM_MEL_COMPUTE.  Its own: the row -> clip
// lookup, the chunked table fetches, the fp64 transposes (lds_read16_b64) and the final store, whose rows are global (vm)
// instead of per clip.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef LW_WPB
#define LW_WPB 4  // waves per workgroup: they share the Hann block and nothing else.  Chosen on the PIPELINED step, where the
#endif            // front end runs beside two CRNN workgroups: 40.83 us at 2 waves, 40.22 at 4 (nothing shared), 39.70 at 4 with
// the Hann block (profiles/EXPERIMENTS.md, section 24; why 4 sits better there is not known).  The kernel ALONE is slower at 4: same
// box, rocprofv3, 256 / 4,096 clips, nothing shared: 4 waves 27.96 / 353.5 us, 2 waves 27.2-27.5 / 350.5-352.0.
// The Hann block behind the per-wave buffers: the half table of 128 pairs (h[2n], h[2n+1]) as the global table holds it, 2,048 B.
// Thread t < 128 fetches pair t beside its wave's samples and parks it; ONE barrier, and every Hann pair of the transform is a
// ds_read_b128 at an immediate offset from one of two per-lane addresses (a 16-lane row reads 256 contiguous bytes: no conflict).
// 4 x 8,704 + 2,048 = 36,864 B per workgroup: four workgroups on a CU alone, one beside two crnn_fused_kernel workgroups at any
// allocation granule up to 2 KB - the sixteen and the four waves that fitted before.  The W512 and W256 twiddles stay in L1: with
// them the block no longer fits beside the CRNN, and the step gains nothing (section 24).
#define LW_HANN_N 128
static_assert(LW_HANN_N <= 64 * LW_WPB, "one 16-byte load per thread fills the Hann block");

#ifndef LW_HC
#define LW_HC 4    // Hann pairs fetched per chunk (16 / LW_HC chunks, double-buffered; sized when the pairs came through L1 and kept for
                   // the LDS block: chunks of 2 or 8 spill registers, section 24)
#endif
#ifndef LW_TC
#define LW_TC 3    // inter-pass twiddles fetched per chunk (15 / LW_TC chunks, double-buffered)
#endif
#ifndef LW_VGPR
#define LW_VGPR 52  // amdgpu_num_vgpr counts in units of two on gfx90a+: 104 registers
#endif
#define LW_WBUF (4 * 16 * TR_LD * 8)  // 8,704 B per wave: 16x16 fp64 transposes of 4 frames; before that the sample tile
#define LW_ROWF 528                   // generic path: floats per staged frame (512 + up to 7 of shift, 16-byte multiple)
static_assert(4 * LW_ROWF * 4 <= LW_WBUF && (WIN + 3 * 512 + 16) * 4 <= LW_WBUF && 4 * MAG_LD * 4 <= LW_WBUF, "per-wave buffer too small");

// The lane number, recomputed where it is needed (two instructions) instead of kept in a register across the transform:
// volatile, so the compiler cannot merge it with an earlier copy and carry that one through the register-tight phases.
__device__ __forceinline__ int lw_lane() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

__device__ __forceinline__ int64_t lw_readlane64(int64_t v, int src_lane) {
  const int lo = __builtin_amdgcn_readlane((int)(v & 0xffffffffll), src_lane);
  const int hi = __builtin_amdgcn_readlane((int)(v >> 32), src_lane);
  return ((int64_t)hi << 32) | (unsigned int)lo;
}

__device__ __forceinline__ int lw_readlane64(int v, int src_lane) { return __builtin_amdgcn_readlane(v, src_lane); }

// Entry e of the Hann block as an LDS pointer the compiler knows nothing about (see lds_opaque), and hann_pair on the block:
// pf = entry j, pr = entry 15 - j
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const f64x2 lds_cf64x2;
__device__ __forceinline__ lds_cf64x2 *lw_hann_entry(const unsigned char *blk, int e) {
  unsigned p = (unsigned)(uintptr_t)blk + 16u * (unsigned)e;  // low 32 bits of a flat LDS pointer = the LDS byte address
  asm volatile("" : "+v"(p));
  return (lds_cf64x2 *)(uintptr_t)p;
}
__device__ __forceinline__ double2 lw_hann_pair(lds_cf64x2 *pf, lds_cf64x2 *pr, int n1) {
  const f64x2 t = n1 < 8 ? pf[16 * n1] : pr[16 * (15 - n1)];
  return n1 < 8 ? make_double2(t.x, t.y) : make_double2(t.y, t.x);
}
template <bool SMALL> struct lw_idx { typedef int64_t type; };
template <> struct lw_idx<true> { typedef int type; };  // every sample index of the launch fits 31 bits (the host checked)

// SMALL: sample indices in 32 bits and (equal clips) the row -> clip division as one multiply: the index arithmetic of a wave
// is vector instructions like everything else, ~100 of the ~960 it issues in 64-bit form.
template <bool F32IN, bool SIMPLE, bool SMALL = false>
__global__ __launch_bounds__(64 * LW_WPB) __attribute__((amdgpu_num_vgpr(LW_VGPR))) void logmel_rows_kernel(logmel_args a) {
  extern __shared__ __align__(16) unsigned char smem[];
  typedef double R;
  constexpr int VEC = F32IN ? 4 : 8;  // elements per 16-byte load
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform values in SGPRs
  const int j = lane & 15, sub = lane >> 4;
  // XCD-aware order: workgroup ids go round-robin to the 8 XCDs; ids of one residue get one contiguous eighth of the
  // frames, so the 352 samples consecutive waves share are fetched through one L2
  const int nper = gridDim.x >> 3;
  const int64_t W = ((int64_t)(blockIdx.x & 7) * nper + (blockIdx.x >> 3)) * LW_WPB + wave;
  const int64_t g0 = W * 4;
  // this thread's pair of the Hann block, requested in front of the wave's samples: the two round trips overlap.  A wave without
  // rows (g0 past the launch's last row: rv below is false in every lane) parks its share, passes the one barrier and leaves
  unsigned char *hblk = smem + (size_t)LW_WPB * LW_WBUF;
  uint4 hv = make_uint4(0, 0, 0, 0);
  if ((int)threadIdx.x < LW_HANN_N) hv = ((const uint4 *)a.hann)[threadIdx.x];
  unsigned char *wb = smem + (size_t)wave * LW_WBUF;
  float *tile = (float *)wb;

  // ---- which clip does this 16-lane row's frame belong to, and where do its samples start
  typedef typename lw_idx<SMALL>::type idx_t;
  idx_t s_begin, b;
  bool rv;
  {
    const int64_t g = g0 + sub;
    rv = g < a.total_frames;
    const int64_t gc = rv ? g : g0;
    if (SMALL && a.uni_magic) {
      // equal clips of >= 4 frames back to back: the wave's first row is a scalar, its clip comes out of one multiply, and a
      // row of the wave is in that clip or the next one
      const unsigned g0u = (unsigned)g0, nfu = (unsigned)a.uniform_nf;
      const unsigned u0 = __umulhi(g0u, a.uni_magic) >> a.uni_shift;
      unsigned f = g0u - u0 * nfu + (unsigned)sub;
      const bool next = f >= nfu;
      f -= next ? nfu : 0u;
      s_begin = (idx_t)((u0 + (next ? 1u : 0u)) * (unsigned)a.uniform_ns);
      b = s_begin + (idx_t)(f * (unsigned)a.hop);  // (rows past the launch's last one get the first row's values below)
    } else if (a.uniform_nf > 0) {  // equal-length clips back to back: arithmetic
      const unsigned gu = (unsigned)gc, nfu = (unsigned)a.uniform_nf;
      const unsigned u = gu / nfu, f = gu - u * nfu;
      s_begin = (idx_t)((int64_t)u * a.uniform_ns);
      b = s_begin + (idx_t)(f * (unsigned)a.hop);
    } else {
      int lo = 0, hi = a.n_utt;  // the last clip whose first mel row is <= g
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.frame_offs[mid] <= gc) lo = mid; else hi = mid;
      }
      const int64_t sb = a.sample_offs[lo];
      const int64_t f = gc - a.frame_offs[lo];
      const int64_t bb = sb + f * a.hop;
      rv = rv && f >= 0 && bb + WIN <= a.sample_offs[lo + 1];  // a row the offset tables do not cover is never stored
      s_begin = (idx_t)sb;
      b = (idx_t)bb;
    }
  }
  const unsigned long long vm = __ballot(rv);
  const float *src = tile;
  int r_last = 0;
  if (vm != 0) {  // (a wave without rows has nothing to stage)
    const int r_first = __builtin_ctzll(vm) >> 4;
    r_last = (63 - __builtin_clzll(vm)) >> 4;
    const idx_t b0 = lw_readlane64(b, 16 * r_first), s0 = lw_readlane64(s_begin, 16 * r_first);
    if (!rv) {  // surplus rows recompute the first valid frame (results unused)
      b = b0;
      s_begin = s0;
    }
    const idx_t total = (idx_t)a.sample_offs[a.n_utt];
    // one contiguous tile serves the wave when every row starts within 3 hops of the first one, in the same clip
    const bool contig = __all(s_begin == s0 && b >= b0 && b - b0 <= 3 * (idx_t)a.hop);
    if (contig) {
      const idx_t bmax = lw_readlane64(b, 16 * r_last);
      const int shift = (int)(b0 % VEC);
      const idx_t ga = b0 - shift;  // multiple of VEC, >= 0
      const int n_vec = (shift + (int)(bmax - b0) + WIN + VEC - 1) / VEC;
      if (SIMPLE) {
        // No pre-emphasis, divisor 32767/32768, hop <= 168 (host checks): NV vectors per lane, straight-line: all loads in
        // flight together
        constexpr int NV = F32IN ? 4 : 2;
        idx_t gq[NV];
        uint4 raw[NV];
        LM_STAGE_SIMPLE_LOAD(F32IN, NV, 64, idx_t, a, ga, n_vec, total, lane, gq, raw);
        LM_STAGE_SIMPLE_STORE(F32IN, NV, 64, idx_t, a, tile, n_vec, total, lane, gq, raw);
      } else {
        stage_generic_wave<F32IN>(a, tile, (int64_t)ga, n_vec, (int64_t)s0, (int64_t)total, lane);
      }
      src = tile + shift + (int)(b - b0);
    } else {
      // frames of two clips (or a very short one) in this wave: frame by frame
      for (int r = 0; r < 4; ++r) {
        if (!((vm >> (16 * r)) & 1)) continue;
        const int64_t br = lw_readlane64(b, 16 * r), sr = lw_readlane64(s_begin, 16 * r);
        const int sh = (int)(br % VEC);
        stage_generic_wave<F32IN>(a, tile + r * LW_ROWF, br - sh, (sh + WIN + VEC - 1) / VEC, sr, (int64_t)total, lane);
      }
      src = tile + (rv ? sub : r_first) * LW_ROWF + (int)(b % VEC);
    }
  }
  if ((int)threadIdx.x < LW_HANN_N) ((uint4 *)hblk)[threadIdx.x] = hv;
  __syncthreads();  // the only barrier: behind it the waves share nothing but the (constant) Hann block
  if (vm == 0) return;
  lds_fence();

  // ---- FFT: every 16-lane row of the wave owns one frame
  R *tr = (R *)wb;          // [4][16][TR_LD]
  float *mg = (float *)wb;  // overlay: [4][MAG_LD]
  cplx<R> v[16];
  lm_mel_fetch mq;  // the mel tail's tables, requested under the untangling
  const double2 *twp = (const double2 *)a.tw16 + j;  // [k1][16 j] = W256^(j k1)
  double2 tq[2][LW_TC];
  {
    // pass 1: lane j holds z[16 n1 + j], n1 = 0..15; Hann product in fp64 (tflite.py:175).  Hann pairs (h[2n], h[2n+1]),
    // n = 16 n1 + j, from the half table of 128 pairs (h[m] = h[511 - m]) in the Hann block, four n1 at a time and one
    // chunk ahead: 16 + 16 registers instead of the 64 of the whole set
    lds_cf64x2 *pf = lw_hann_entry(hblk, j), *pr = lw_hann_entry(hblk, 15 - j);
    constexpr int HC = LW_HC, NHC = 16 / HC;  // Hann pairs per chunk; one chunk in flight ahead of the one being used
    double2 h[2][HC];
#pragma unroll
    for (int i = 0; i < HC; ++i) h[0][i] = lw_hann_pair(pf, pr, i);
    const bool pairs = __all((((int)(src - tile)) & 1) == 0);
    if (pairs) {
      // 8-byte aligned pairs: ds_read_b64 (with hop = 160 the four frames of a wave sit 32 banks apart: conflict-free)
      double xs[16];
      lds_read16_b64_s128(src + 2 * j, xs);
#pragma unroll
      for (int c = 0; c < NHC; ++c) {
        if (c + 1 < NHC) {
#pragma unroll
          for (int i = 0; i < HC; ++i) h[(c + 1) & 1][i] = lw_hann_pair(pf, pr, HC * (c + 1) + i);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c == 0) lds_wait_all(xs);
#pragma unroll
        for (int i = 0; i < HC; ++i) v[HC * c + i] = hann_mul_pair<R>(xs[HC * c + i], h[c & 1][i]);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
      for (int c = 0; c < NHC; ++c) {
        if (c + 1 < NHC) {
#pragma unroll
          for (int i = 0; i < HC; ++i) h[(c + 1) & 1][i] = lw_hann_pair(pf, pr, HC * (c + 1) + i);
        }
#pragma unroll
        for (int i = 0; i < HC; ++i) v[HC * c + i] = hann_mul_at<R>(src, 16 * (HC * c + i) + j, h[c & 1][i]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  {
    // the first inter-pass twiddles are requested before the butterflies that precede their use
    constexpr int TC = LW_TC, NTC = 15 / TC;
#pragma unroll
    for (int i = 0; i < TC; ++i) tq[0][i] = twp[k_of(1 + i) * 16];
    dft16<R>(v);
    // v[pos] *= W256^(j k_of(pos)): 15 sixteen-byte loads per lane from the L1-resident table, TC at a time, one chunk ahead
#pragma unroll
    for (int c = 0; c < NTC; ++c) {
      if (c + 1 < NTC) {
#pragma unroll
        for (int i = 0; i < TC; ++i) tq[(c + 1) & 1][i] = twp[k_of(1 + TC * (c + 1) + i) * 16];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TC; ++i) {
        const int pos = 1 + TC * c + i;
        v[pos] = cmul(v[pos], cplx<R>{tq[c & 1][i].x, tq[c & 1][i].y});
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // 16x16 transpose through LDS, real parts then imaginary parts (same buffer)
    cplx<R> w[16];
    const int l2 = lw_lane(), j = l2 & 15, sub = l2 >> 4;
    R *trs = tr + sub * 16 * TR_LD;
#pragma unroll
    for (int pos = 0; pos < 16; ++pos) trs[k_of(pos) * TR_LD + j] = v[pos].re;
    lds_fence();
    {
      double wre[16], wim[16];
      lds_read16_b64((const double *)trs + j * TR_LD, wre);
      lds_fence();
#pragma unroll
      for (int pos = 0; pos < 16; ++pos) trs[k_of(pos) * TR_LD + j] = v[pos].im;
      lds_fence();
      lds_read16_b64((const double *)trs + j * TR_LD, wim);
      lds_wait_all(wre);
      lds_wait_all(wim);
#pragma unroll
      for (int n2 = 0; n2 < 16; ++n2) {
        w[n2].re = wre[n2];
        w[n2].im = wim[n2];
      }
    }
    // pass 2: lane j = k1 holds Y[n2][k1]; output w[pos] = Z[k1 + 16 k_of(pos)]
    dft16<R>(w);
    // untangle: the partners Z[256 - k] arrive through the (dead) transpose buffer, W512^k from the L1-resident table two k2 at a
    // time and one chunk ahead
    const double2 *unp = (const double2 *)a.tw512 + j;  // W512^(j + 16 k2) at [16 k2]
    double2 uq[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) uq[0][i] = unp[16 * i];
    // The mel tail's tables ride under the untangling: every request BEHIND the uq request of its chunk, so that the counted
    // wait for a uq chunk never waits for mel data (loads return in order), and each as soon as the registers are there: three
    // meta words now, the biases a chunk later, the weights of groups 0 and 1 (52 registers) behind the third chunk, when twelve
    // of the sixteen w and pz pairs are retired (a chunk earlier they spill).  The generic-staging instances carry more across
    // the transform and have no room for weights before untangle_tail (W_AT 4: requested there).
    constexpr int W_AT = SIMPLE ? 3 : 4;
    __builtin_amdgcn_sched_barrier(0);
    LM_MEL_REQ_META(a, l2, mq);
    cplx<R> pz[8];
    LM_PARTNERS(R, w, trs, j, pz);
    float *mrow = mg + sub * MAG_LD;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c + 1 < 4) {
#pragma unroll
        for (int i = 0; i < 2; ++i) uq[(c + 1) & 1][i] = unp[16 * (2 * (c + 1) + i)];
      }
      if (c == 0 || c == W_AT) {
        __builtin_amdgcn_sched_barrier(0);
        if (c == 0) LM_MEL_REQ_BIAS(a, mq);
        if (c == W_AT) {
          LM_MEL_REQ_W(a, l2, mq, 0);
          LM_MEL_REQ_W(a, l2, mq, 1);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int k2 = 2 * c + i;
        LM_UNTANGLE_K2(R, w[pos_of(k2)], pz[k2], (cplx<R>{uq[c & 1][i].x, uq[c & 1][i].y}), mrow, j + 16 * k2);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    untangle_tail<R>(w[pos_of(8)], mrow, j);
  }

  // ---- mel filterbank and the park of the wave's 4 x n_mel tile.  Mel rows are global frame numbers: the four rows leave as
  //      one contiguous store when all four are valid (16-byte aligned whenever n_mel is a multiple of 4: g0 is a multiple of 4)
  lds_fence();
  {
    const int lane = lw_lane();
    __builtin_amdgcn_sched_barrier(0);
    if (!SIMPLE) {
      LM_MEL_REQ_W(a, lane, mq, 0);
      LM_MEL_REQ_W(a, lane, mq, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    LM_MEL_COMPUTE(a, mg, lane, mq, 2);
    float *dstf = a.mel + g0 * (int64_t)a.n_mel;
    const bool prefix = (vm & (vm + 1)) == 0;  // valid rows are 0 .. r_last
    if (prefix && (((uintptr_t)dstf) & 15) == 0 && (a.n_mel & 3) == 0) {
      const int nv = r_last + 1;
      for (int i = lane; i < nv * a.n_mel / 4; i += 64) ((float4 *)dstf)[i] = ((const float4 *)mg)[i];
    } else {
      for (int i = lane; i < 4 * a.n_mel; i += 64)
        if ((vm >> (16 * (i / a.n_mel))) & 1) dstf[i] = mg[i];
    }
  }
}

#define STFT_MAG_LD 260  // floats per frame of magnitudes outside the log-mel kernels: 257, padded to a 16-byte multiple
// stft_mag_kernel's dynamic LDS: per wave the FFT buffer, then the magnitudes
template <typename R>
struct stft_mag_lds {
  static constexpr size_t mag = WAVES * FFT_LD * sizeof(cplx<R>);
  static constexpr size_t bytes = mag + WAVES * STFT_MAG_LD * sizeof(float);
};

// STFT magnitude of explicit frames [n][512] -> [n][257]; one wave per frame.
template <typename R>
__global__ __launch_bounds__(256) void stft_mag_kernel(logmel_args a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  cplx<R> *fbuf = (cplx<R> *)smem;
  float *mag = (float *)(smem + stft_mag_lds<R>::mag);
  fft_consts<R> fc;
  fft_load_consts<R>(fc, lane, a.hann, a.tw256, a.tw512);
  const int64_t f = (int64_t)blockIdx.x * WAVES + wave;
  if (f >= a.n_frames_direct) return;
  const float *src = a.frames + f * WIN;
  auto x2 = [&](int n) -> float2 { return *(const float2 *)(src + 2 * n); };
  float *mg = mag + wave * STFT_MAG_LD;
  frame_fft_mag<R>(x2, fc, fbuf + wave * FFT_LD, mg, lane);
  float *dst = a.mag_out + f * NB;
  for (int k = lane; k < NB; k += 64) dst[k] = mg[k];
}

static void fill_filter_args(logmel_args &a, const ww_model *m) {
  const ww_filter_dev &f = m->filt;
  a.start = f.start; a.wpad = f.wpad; a.bias = f.bias;
  a.n_mel = f.n_mel;
  a.floor_v = f.floor_v; a.log_off = f.log_off; a.scale = f.scale;
  a.hann = f.hann; a.tw256 = f.tw256; a.tw512 = f.tw512; a.tw16 = f.tw16;
  a.melV = f.melV; a.melVmeta = f.melVmeta; a.melv_aligned = f.melv_aligned;
}

// The instantiation for an input type and a staging form: straight-line staging (`simple`) when nothing exotic is asked for,
// for logmel_rows_kernel also with 32-bit sample indices (`small_idx`, which implies `simple`)
typedef void (*logmel_fn)(logmel_args);
static logmel_fn logmel_instance(bool rows, bool f32in, bool simple, bool small_idx) {
  static const logmel_fn tile[2][2] = {{logmel_kernel<false, false>, logmel_kernel<true, false>},
                                       {logmel_kernel<false, true>, logmel_kernel<true, true>}};
  static const logmel_fn wave[3][2] = {{logmel_rows_kernel<false, false>, logmel_rows_kernel<true, false>},
                                       {logmel_rows_kernel<false, true>, logmel_rows_kernel<true, true>},
                                       {logmel_rows_kernel<false, true, true>, logmel_rows_kernel<true, true, true>}};
  return rows ? wave[simple + (simple && small_idx)][f32in] : tile[simple][f32in];
}

int ww_k_logmel(ww_ctx *ctx, const ww_model *m, const int16_t *d_pcm, const float *d_f32, const int64_t *d_sample_offs,
                const int64_t *d_frame_offs, int n_utt, int64_t total_frames, int64_t max_frames_per_utt,
                const ww_frontend_params *fp, float *d_mel, int64_t uniform_samples, int64_t total_samples_hint) {
  if (n_utt <= 0 || total_frames <= 0 || max_frames_per_utt <= 0) return WW_OK;
  if (fp->hop <= 0 || fp->hop > 512) return ww_fail(ctx, WW_EINVAL, "hop %d out of range (1..512)", fp->hop);
  logmel_args a = {};
  a.pcm = d_pcm; a.f32 = d_f32; a.sample_offs = d_sample_offs; a.frame_offs = d_frame_offs;
  a.n_utt = n_utt; a.hop = fp->hop; a.divisor = fp->pcm_divisor; a.clip = fp->clip; a.preemph = fp->pre_emphasis;
  a.rdiv = 1.0f / fp->pcm_divisor;
  a.fast_div = (fp->pcm_divisor == 32767.0f || fp->pcm_divisor == 32768.0f) ? 1 : 0;
  a.mel = d_mel;
  fill_filter_args(a, m);
  const bool f32in = d_f32 != nullptr;
  // straight-line staging when nothing exotic is asked for and the tile fits the kernel's vectors per thread: two for each of
  // logmel_kernel's 256 threads, NV for each of logmel_rows_kernel's 64 lanes (hop <= 168)
  const bool plain = fp->pre_emphasis == 0.0f && (f32in || a.fast_div);
  const bool simple = plain && WIN + (FPB - 1) * fp->hop + 16 <= 512 * (f32in ? 4 : 8);
  if (fp->precise) {
    // fp64: waves own four consecutive global mel rows each (logmel_rows_kernel)
    a.total_frames = total_frames;
    if (uniform_samples > 0 && total_frames < 0x7fffffff && total_frames == (int64_t)n_utt * max_frames_per_utt) {
      a.uniform_nf = (int)max_frames_per_utt;
      a.uniform_ns = uniform_samples;
    }
    const bool simple_w = plain && fp->hop <= 168;
    // 32-bit sample indices when the caller could tell that every index of the launch fits 31 bits; with equal clips of >= 4
    // frames the row -> clip division becomes one multiply: M = ceil(2^(31 + l) / nf), l = ceil(log2 nf), is exact for
    // every row < 2^31 (M nf - 2^(31 + l) < nf <= 2^l)
    const bool small_w = simple_w && total_samples_hint > 0 && total_samples_hint < 0x7fff0000ll;
    if (small_w && a.uniform_nf >= 4) {
      int l = 0;
      while ((1ll << l) < a.uniform_nf) ++l;
      a.uni_magic = (unsigned)(((1ull << (31 + l)) + (unsigned)a.uniform_nf - 1) / (unsigned)a.uniform_nf);
      a.uni_shift = l - 1;
    }
    const int64_t n_waves = (total_frames + 3) / 4;
    const int64_t n_wg = 8 * ((((n_waves + LW_WPB - 1) / LW_WPB) + 7) / 8);
    if (n_wg > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "front-end launch too large (%lld workgroups): split the batch", (long long)n_wg);
    const dim3 grid_w((unsigned)n_wg), block_w(64 * LW_WPB);
    const size_t sm = (size_t)LW_WPB * LW_WBUF + LW_HANN_N * 16;  // per-wave buffers, Hann block
    ww_launch_scope scope(ctx, "logmel_rows_kernel");
    hipLaunchKernelGGL(logmel_instance(true, f32in, simple_w, small_w), grid_w, block_w, sm, ctx->stream, a);
    WW_HIP(ctx, hipGetLastError());
    return WW_OK;
  }
  const int64_t tiles = (max_frames_per_utt + FPB - 1) / FPB;
  const int64_t n_ids = 8 * (((int64_t)n_utt + 7) / 8) * tiles;
  if (n_ids > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "front-end launch too large (%lld workgroups): split the batch", (long long)n_ids);
  a.tiles_per_utt = (int)tiles;
  dim3 grid((unsigned)n_ids);
  ww_launch_scope scope(ctx, "logmel_kernel<f32>");
  hipLaunchKernelGGL(logmel_instance(false, f32in, simple, false), grid, dim3(256), logmel_lds::bytes(fp->hop), ctx->stream, a);
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

// filter.tflite alone (reference filter_model(frame), wakeword/tflite.py:183-184): mag [n][257] -> mel [n][40]
__global__ __launch_bounds__(64) void mel_only_kernel(const float *mag, int64_t n, const float *w, const float *bias, int n_mel,
                                                      int n_bins, float floor_v, float log_off, float scale, float *mel) {
  __shared__ float m[STFT_MAG_LD];
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  for (int k = lane; k < n_bins; k += 64) m[k] = mag[f * n_bins + k];
  __syncthreads();
  if (lane < n_mel) {
    float acc = 0.f;
    for (int k = 0; k < n_bins; ++k) acc = fmaf(w[(size_t)lane * n_bins + k], m[k], acc);
    acc = fmaxf(acc + bias[lane], floor_v);
    mel[f * n_mel + lane] = (logf(acc) + log_off) * scale;
  }
}

int ww_k_mel_only(ww_ctx *ctx, const ww_model *m, const float *d_mag, int64_t n, float *d_mel) {
  if (n <= 0) return WW_OK;
  const ww_filter_dev &f = m->filt;
  ww_launch_scope scope(ctx, "mel_only_kernel");
  hipLaunchKernelGGL(mel_only_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, d_mag, n, f.wdense, f.bias, f.n_mel, f.n_bins,
                     f.floor_v, f.log_off, f.scale, d_mel);
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

int ww_k_stft_mag(ww_ctx *ctx, const ww_model *m, const float *d_frames, int64_t n, int precise, float *d_mag) {
  if (n <= 0) return WW_OK;
  logmel_args a = {};
  fill_filter_args(a, m);
  a.frames = d_frames; a.mag_out = d_mag; a.n_frames_direct = n;
  dim3 grid((unsigned)((n + WAVES - 1) / WAVES));
  ww_launch_scope scope(ctx, "stft_mag_kernel");
  if (precise) hipLaunchKernelGGL((stft_mag_kernel<double>), grid, dim3(256), stft_mag_lds<double>::bytes, ctx->stream, a);
  else hipLaunchKernelGGL((stft_mag_kernel<float>), grid, dim3(256), stft_mag_lds<float>::bytes, ctx->stream, a);
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}
