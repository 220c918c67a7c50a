// Rational-ratio polyphase windowed-sinc resampler (include/wwhip.h: ww_resample*): audio at any rate -> the models' 16 kHz.
//
//   y[m] = sum_k h[m * down - k * up] * x[k],  |m * down - k * up| <= half
//
// Arithmetic rule (as for the models): an output is ONE fmaf chain from +0 over its input samples in ascending k,
// every tap rounded once from float64.  Taps outside the filter are stored as +0 and samples outside the segment are staged as
// +0: fmaf(0, x, acc) and fmaf(h, 0, acc) leave acc as it is, so padding a chain changes no bit, and neither does the choice of
// kernel form, tile, launch or packet cut.
//
// Two forms, both with a tile's input span staged once in LDS as fp32 (int16 converted there):
//   up == 1 (48, 32, 96 kHz -> 16 kHz: every output has the same taps): a lane owns RS_R1 consecutive outputs and walks its input
//     window once - each staged sample is read from LDS once and feeds all RS_R1 chains; the RS_R1 taps that go with window
//     position u are one row of a host-built table [n_u][8], a wave-uniform address (scalar loads).
//   any up (44.1, 22.05, 11.025, 8 kHz ...): outputs are grouped by phase.  Item e = A * up + p owns the R outputs
//     m = (A * R + r) * up + q(p), r < R, which share phase p = m * down mod up: one tap load feeds R chains.  Lanes are
//     consecutive in p, and the table is tap-major [tpp][up], so a wave's tap load is one coalesced row segment.  R = 8 for long
//     output ranges, R = 1 for short ones (a stream's packets), where R * up outputs per item would mostly be idle.
#include "common.h"

#include <algorithm>
#include <cmath>

#define RS_THREADS 256
#define RS_UNROLL1 4                  // window positions per unrolled step of the up == 1 form (the table is padded to it)
// (tile descriptor rs_tile, RS_XCAP / RS_R / RS_R1 / RS_COPY and the tile plans: launch_plan.h)

struct ww_resampler : rs_geom {
  ww_ctx *ctx = nullptr;
  int32_t rate_in = 0, rate_out = 0;
  int64_t dinv = 0;
  float *d_taps = nullptr;  // [tpp][up] tap-major
  float *d_h2 = nullptr;    // up == 1: [n_u][8], row u = the taps of outputs r = 0 .. RS_R1 - 1 at window position u
  size_t table_bytes = 0;
};

__device__ __forceinline__ float rs_load(int16_t v) { return (float)v * (1.0f / 32768.0f); }  // exact: a power of two
__device__ __forceinline__ float rs_load(float v) { return v; }
// G.711 (ITU-T, 16-bit output: audioop.ulaw2lin / alaw2lin at width 2): a code decodes in registers to the int16 sample, which goes the
// int16 sample's way from there on - the chains see the same fp32 values, so a G.711 input yields the decoded int16 input's bits.
struct rs_mulaw { uint8_t code; };
struct rs_alaw { uint8_t code; };
__host__ __device__ __forceinline__ int g711_mulaw(unsigned code) {
  const unsigned v = ~code & 0xFFu;
  const int t = (int)((((v & 0x0Fu) << 3) + 0x84u) << ((v & 0x70u) >> 4));
  return (v & 0x80u) ? 0x84 - t : t - 0x84;
}
__host__ __device__ __forceinline__ int g711_alaw(unsigned code) {
  const unsigned v = (code ^ 0x55u) & 0xFFu, seg = (v & 0x70u) >> 4;
  int t = (int)((v & 0x0Fu) << 4);
  t = seg == 0 ? t + 8 : (t + 0x108) << (seg - 1);
  return (v & 0x80u) ? t : -t;
}
__host__ __device__ __forceinline__ int g711_decode(int law, unsigned code) { return law == WW_SAMPLE_MULAW ? g711_mulaw(code) : g711_alaw(code); }
__device__ __forceinline__ float rs_load(rs_mulaw v) { return rs_load((int16_t)g711_mulaw(v.code)); }
__device__ __forceinline__ float rs_load(rs_alaw v) { return rs_load((int16_t)g711_alaw(v.code)); }
__device__ __forceinline__ void rs_store(float *p, float v) { *p = v; }
__device__ __forceinline__ void rs_store(int16_t *p, float v) {
  v = rintf(v * 32768.0f);
  v = fminf(fmaxf(v, -32768.0f), 32767.0f);
  *p = (int16_t)(int)v;
}

template <typename TIn>
__device__ __forceinline__ void rs_stage(float *xs, const TIn *__restrict__ in, const rs_tile &t) {
  const TIn *seg = in + t.in_off;
  const int64_t d = t.k_lo - t.in_first;  // segment index of staged sample 0
  for (int i = threadIdx.x; i < t.n_x; i += RS_THREADS) {
    const int64_t j = d + i;
    float v = 0.0f;
    if (j >= 0 && j < t.n_in) v = rs_load(seg[j]);
    xs[i] = v;
  }
}

template <typename TIn, typename TOut>
__global__ __launch_bounds__(RS_THREADS) void resample_copy_kernel(const TIn *__restrict__ in, TOut *__restrict__ out,
                                                                   const rs_tile *__restrict__ tiles) {
  const rs_tile t = tiles[blockIdx.x];
  for (int i = threadIdx.x; i < t.n; i += RS_THREADS) {
    const int64_t m = t.first + i, j = m - t.in_first;
    float v = 0.0f;
    if (j >= 0 && j < t.n_in) v = rs_load(in[t.in_off + j]);
    rs_store(out + t.out_off + (m - t.out_first), v);
  }
}

template <typename TIn, typename TOut>
__global__ __launch_bounds__(RS_THREADS) void resample_decim_kernel(const TIn *__restrict__ in, TOut *__restrict__ out,
                                                                    const rs_tile *__restrict__ tiles, const float *__restrict__ h2,
                                                                    int down, int n_u) {
  __shared__ float xs[RS_XCAP];
  const rs_tile t = tiles[blockIdx.x];
  rs_stage(xs, in, t);
  __syncthreads();
  if ((int)threadIdx.x >= t.n) return;
  const float *x0 = xs + (int)threadIdx.x * RS_R1 * down;  // t.k_lo = t.first * down - half: this lane's window position 0
  float acc[RS_R1];
#pragma unroll
  for (int r = 0; r < RS_R1; ++r) acc[r] = 0.0f;
  for (int u = 0; u < n_u; u += RS_UNROLL1) {
#pragma unroll
    for (int v = 0; v < RS_UNROLL1; ++v) {
      const float xv = x0[u + v];
      const float *hh = h2 + (size_t)(u + v) * 8;  // the same address in every lane
#pragma unroll
      for (int r = 0; r < RS_R1; ++r) acc[r] = fmaf(hh[r], xv, acc[r]);
    }
  }
  const int64_t m0 = t.first + (int64_t)threadIdx.x * RS_R1;
#pragma unroll
  for (int r = 0; r < RS_R1; ++r)
    if (m0 + r < t.out_end) rs_store(out + t.out_off + (m0 + r - t.out_first), acc[r]);
}

// The phase form's chain, shared with the stream banks' tick (stream_rate_tick_kernel): tap 0 of phase p is h[p + jmax * up], the
// largest index <= half of the phase, and the R outputs of one item, `down` staged samples apart, take tap tt (tp[tt * up], tp =
// taps + p) over x0[r * down + tt] in ascending tt - ascending k.
__device__ __forceinline__ int rs_jmax(int half, int p, int up) { return (half - p) / up; }
template <int R>
__device__ __forceinline__ void rs_chains(float (&acc)[R], const float *x0, const float *tp, int up, int down, int tpp) {
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0f;
#pragma unroll 8
  for (int tt = 0; tt < tpp; ++tt) {
    const float h = tp[(size_t)tt * up];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = fmaf(h, x0[r * down + tt], acc[r]);
  }
}

template <int R, typename TIn, typename TOut>
__global__ __launch_bounds__(RS_THREADS) void resample_phase_kernel(const TIn *__restrict__ in, TOut *__restrict__ out,
                                                                    const rs_tile *__restrict__ tiles, const float *__restrict__ taps,
                                                                    int up, int down, int half, int tpp, int dinv) {
  __shared__ float xs[RS_XCAP];
  const rs_tile t = tiles[blockIdx.x];
  rs_stage(xs, in, t);
  __syncthreads();
  if ((int)threadIdx.x >= t.n) return;
  const int64_t e = t.first + threadIdx.x;
  const int64_t A = e / up;
  const int p = (int)(e - A * up);                     // phase: m * down mod up of every output of this item
  const int q = (int)(((int64_t)p * dinv) % up);       // m mod up
  const int cq = (int)(((int64_t)q * down) / up);      // floor(m * down / up) = (m / up) * down + cq
  const int jmax = rs_jmax(half, p, up);
  const float *x0 = xs + (int)(A * R * down + cq - jmax - t.k_lo);  // sample of tap 0 of output r = 0
  float acc[R];
  rs_chains<R>(acc, x0, taps + p, up, down, tpp);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t m = (A * R + r) * up + q;
    if (m >= t.out_first && m < t.out_end) rs_store(out + t.out_off + (m - t.out_first), acc[r]);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
static double rs_i0(double x) {  // modified Bessel function I0 by its power series (every term positive: no cancellation)
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < sum * 1e-18) break;
  }
  return sum;
}

static int64_t rs_gcd(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

static int64_t rs_inverse(int64_t a, int64_t n) {  // a^-1 mod n, gcd(a, n) = 1
  int64_t t = 0, nt = 1, r = n, nr = a % n;
  while (nr) {
    const int64_t qq = r / nr, t2 = t - qq * nt, r2 = r - qq * nr;
    t = nt; nt = t2; r = nr; nr = r2;
  }
  return t < 0 ? t + n : t;
}

template <typename K, typename... Args>
static void rs_launch(ww_ctx *ctx, const char *name, K kernel, size_t n_tiles, Args... args) {
  ww_launch_scope scope(ctx, name);
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_tiles), dim3(RS_THREADS), 0, ctx->stream, args...);
}

static size_t rs_sample_bytes(int fmt) {  // 0: not a sample format
  return fmt == WW_SAMPLE_I16 ? 2 : fmt == WW_SAMPLE_F32 ? 4 : (fmt == WW_SAMPLE_MULAW || fmt == WW_SAMPLE_ALAW) ? 1 : 0;
}

static int rs_validate(const ww_resampler *r, const void *in, int in_fmt, const int64_t *so, const int64_t *in_first, const int64_t *out_first,
                       const int64_t *oo, int n_seg, const void *out, int out_fmt, int64_t *n_out_total) {
  ww_ctx *ctx = r->ctx;
  *n_out_total = 0;
  if (n_seg < 0) return ww_fail(ctx, WW_EINVAL, "ww_resample: n_seg = %d", n_seg);
  if (out_fmt == WW_SAMPLE_MULAW || out_fmt == WW_SAMPLE_ALAW)
    return ww_fail(ctx, WW_EINVAL, "ww_resample: G.711 is an input format only: out_format is WW_SAMPLE_I16 or WW_SAMPLE_F32");
  if (rs_sample_bytes(in_fmt) == 0 || (out_fmt != WW_SAMPLE_I16 && out_fmt != WW_SAMPLE_F32))
    return ww_fail(ctx, WW_EINVAL, "ww_resample: sample formats are WW_SAMPLE_I16 and WW_SAMPLE_F32 (in_format: also WW_SAMPLE_MULAW and WW_SAMPLE_ALAW)");
  if (n_seg == 0) return WW_OK;
  if (!so || !oo) return ww_fail(ctx, WW_EINVAL, "ww_resample: NULL offset table");
  if (so[0] < 0 || oo[0] < 0) return ww_fail(ctx, WW_EINVAL, "ww_resample: negative offset");
  for (int u = 0; u < n_seg; ++u) {
    if (so[u + 1] < so[u] || oo[u + 1] < oo[u]) return ww_fail(ctx, WW_EINVAL, "ww_resample: descending offsets at segment %d", u);
    const int64_t i0 = in_first ? in_first[u] : 0, o0 = out_first ? out_first[u] : 0;
    if (i0 < 0 || o0 < 0) return ww_fail(ctx, WW_EINVAL, "ww_resample: negative in_first / out_first at segment %d", u);
    const int64_t cnt = oo[u + 1] - oo[u], lim = rs_out_len(r, i0 + (so[u + 1] - so[u]));
    if (cnt > 0 && o0 + cnt > lim)
      return ww_fail(ctx, WW_EINVAL, "ww_resample: segment %d asks for outputs [%lld, %lld) of a signal that has %lld", u, (long long)o0,
                     (long long)(o0 + cnt), (long long)lim);
  }
  *n_out_total = oo[n_seg] - oo[0];
  if (*n_out_total > 0 && !out) return ww_fail(ctx, WW_EINVAL, "ww_resample: NULL output buffer");
  if (*n_out_total > 0 && so[n_seg] > so[0] && !in) return ww_fail(ctx, WW_EINVAL, "ww_resample: NULL input buffer");
  return WW_OK;
}

template <typename TIn, typename TOut>
static void rs_launch_all(const ww_resampler *r, const rs_plan &pl, const rs_tile *d_tiles, const TIn *d_in, TOut *d_out) {
  ww_ctx *ctx = r->ctx;
  const rs_tile *d = d_tiles;
  if (!pl.copy.empty()) rs_launch(ctx, "resample_copy_kernel", resample_copy_kernel<TIn, TOut>, pl.copy.size(), d_in, d_out, d);
  d += pl.copy.size();
  if (!pl.decim.empty())
    rs_launch(ctx, "resample_decim_kernel", resample_decim_kernel<TIn, TOut>, pl.decim.size(), d_in, d_out, d, (const float *)r->d_h2, (int)r->down,
              (int)r->n_u);
  d += pl.decim.size();
  if (!pl.ph8.empty())
    rs_launch(ctx, "resample_phase_kernel<8>", resample_phase_kernel<RS_R, TIn, TOut>, pl.ph8.size(), d_in, d_out, d, (const float *)r->d_taps,
              (int)r->up, (int)r->down, (int)r->half, (int)r->tpp, (int)r->dinv);
  d += pl.ph8.size();
  if (!pl.ph1.empty())
    rs_launch(ctx, "resample_phase_kernel<1>", resample_phase_kernel<1, TIn, TOut>, pl.ph1.size(), d_in, d_out, d, (const float *)r->d_taps,
              (int)r->up, (int)r->down, (int)r->half, (int)r->tpp, (int)r->dinv);
}

// the four tile lists are one table, in rs_launch_all's order
static int rs_run(const ww_resampler *r, const rs_plan &pl, rs_tile *d_tiles, const void *d_in, int in_fmt, void *d_out, int out_fmt) {
  ww_ctx *ctx = r->ctx;
  ww_tables tb;
  tb.add(pl.copy);
  tb.join(pl.decim);
  tb.join(pl.ph8);
  tb.join(pl.ph1);
  if (int rc = tb.send(ctx, d_tiles)) return rc;
  auto to = [&](auto *in) {
    if (out_fmt == WW_SAMPLE_F32) rs_launch_all(r, pl, d_tiles, in, (float *)d_out);
    else rs_launch_all(r, pl, d_tiles, in, (int16_t *)d_out);
  };
  if (in_fmt == WW_SAMPLE_I16) to((const int16_t *)d_in);
  else if (in_fmt == WW_SAMPLE_F32) to((const float *)d_in);
  else if (in_fmt == WW_SAMPLE_MULAW) to((const rs_mulaw *)d_in);
  else to((const rs_alaw *)d_in);
  WW_HIP(ctx, hipGetLastError());
  return WW_OK;
}

extern "C" {

int ww_resampler_destroy(ww_resampler *r) {
  WW_GUARD_BEGIN
  if (!r) return WW_OK;
  ww_device_scope dev_scope(r->ctx->device);
  hipStreamSynchronize(r->ctx->stream);
  if (r->d_taps) hipFree(r->d_taps);
  if (r->d_h2) hipFree(r->d_h2);
  delete r;
  return WW_OK;
  WW_GUARD_END(nullptr)
}

int ww_resampler_create(ww_ctx *ctx, int32_t rate_in, int32_t rate_out, const ww_resampler_params *params, ww_resampler **out) {
  WW_GUARD_BEGIN
  if (!ctx || !out) return ww_fail(ctx, WW_EINVAL, "ww_resampler_create: NULL argument");
  *out = nullptr;
  if (rate_in <= 0 || rate_out <= 0) return ww_fail(ctx, WW_EINVAL, "ww_resampler_create: rates must be positive (%d -> %d)", rate_in, rate_out);
  const double rolloff = params ? params->rolloff : 0.945, beta = params ? params->beta : 14.769656459379492;
  const int zeros = params ? params->zeros : 32;
  if (zeros < 1 || !(rolloff > 0.0 && rolloff <= 1.0) || !(beta >= 0.0) || !(beta < 100.0))
    return ww_fail(ctx, WW_EINVAL, "ww_resampler_create: zeros >= 1, 0 < rolloff <= 1 and 0 <= beta < 100 are needed");
  WW_ON_DEVICE(ctx, dev);
  ww_resampler *r = new ww_resampler();
  ww_scoped<ww_resampler, ww_resampler_destroy> own(r);
  r->ctx = ctx;
  r->rate_in = rate_in;
  r->rate_out = rate_out;
  const int64_t g = rs_gcd(rate_in, rate_out);
  const int64_t up = r->up = rate_out / g, down = r->down = rate_in / g;
  if (up == 1 && down == 1) {
    r->identity = true;
    *out = own.release();
    return WW_OK;
  }
  const double L = (double)((int64_t)rate_in * up);
  const double f2 = rolloff * (double)std::min(rate_in, rate_out) / L;
  const double halfd = std::ceil((double)zeros / f2);
  const double tapsd = std::ceil((2.0 * halfd + 1.0) / (double)up) * (double)up;
  if (!(tapsd <= (double)WW_RESAMPLE_MAX_TAPS))
    return ww_fail(ctx, WW_EINVAL, "ww_resampler_create: %d -> %d needs a table of %.0f taps; WW_RESAMPLE_MAX_TAPS is %d", rate_in, rate_out, tapsd,
                   WW_RESAMPLE_MAX_TAPS);
  const int64_t half = r->half = (int64_t)halfd, tpp = r->tpp = (2 * half + 1 + up - 1) / up;
  if (2 * down + tpp + 2 > RS_XCAP)
    return ww_fail(ctx, WW_EINVAL, "ww_resampler_create: %d -> %d needs a tile of %lld staged samples; WW_RESAMPLE_MAX_SPAN is %d", rate_in, rate_out,
                   (long long)(2 * down + tpp + 2), RS_XCAP);
  std::vector<double> h((size_t)(2 * half + 1));
  const double i0b = rs_i0(beta), pi = 3.14159265358979323846;
  for (int64_t i = -half; i <= half; ++i) {
    const double a = (double)i / (double)half, w = rs_i0(beta * std::sqrt(std::max(0.0, 1.0 - a * a))) / i0b;
    const double y = pi * (f2 * (double)i), s = i == 0 ? 1.0 : std::sin(y) / y;
    h[(size_t)(i + half)] = (double)up * f2 * s * w;
  }
  std::vector<float> tab((size_t)(tpp * up));
  for (int64_t p = 0; p < up; ++p) {
    const int64_t jmax = (half - p) / up;
    for (int64_t tt = 0; tt < tpp; ++tt) {
      const int64_t idx = half + p + (jmax - tt) * up;
      tab[(size_t)(tt * up + p)] = idx >= 0 ? (float)h[(size_t)idx] : 0.0f;
    }
  }
  WW_HIP(ctx, hipMalloc((void **)&r->d_taps, tab.size() * 4));
  WW_HIP(ctx, hipMemcpy(r->d_taps, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  r->table_bytes = tab.size() * 4;
  r->dinv = up > 1 ? rs_inverse(down % up, up) : 0;
  for (int64_t ne = RS_THREADS; ne >= 64 && !r->ne8; ne /= 2)
    if (rs_phase_span(r, RS_R, ne) <= RS_XCAP) r->ne8 = (int32_t)ne;
  for (int64_t ne = RS_THREADS; ne >= 1 && !r->ne1; ne /= 2)
    if (rs_phase_span(r, 1, ne) <= RS_XCAP) r->ne1 = (int32_t)ne;
  if (up == 1) {
    const int64_t n_u = (RS_R1 - 1) * down + 2 * half + 1, n_u_pad = (n_u + RS_UNROLL1 - 1) / RS_UNROLL1 * RS_UNROLL1;
    const int64_t lanes = std::min<int64_t>(RS_THREADS, (RS_XCAP - n_u_pad) / (RS_R1 * down) + 1);
    if (n_u_pad <= RS_XCAP && lanes >= 1) {
      std::vector<float> h2((size_t)n_u_pad * 8, 0.0f);
      for (int64_t u = 0; u < n_u; ++u)
        for (int64_t rr = 0; rr < RS_R1; ++rr) {
          const int64_t idx = rr * down + 2 * half - u;
          if (idx >= 0 && idx <= 2 * half) h2[(size_t)(u * 8 + rr)] = (float)h[(size_t)idx];
        }
      WW_HIP(ctx, hipMalloc((void **)&r->d_h2, h2.size() * 4));
      WW_HIP(ctx, hipMemcpy(r->d_h2, h2.data(), h2.size() * 4, hipMemcpyHostToDevice));
      r->n_u = (int32_t)n_u_pad;
      r->lanes1 = (int32_t)lanes;
    }
  }
  *out = own.release();
  return WW_OK;
  WW_GUARD_END(ctx)
}

int ww_resampler_info(const ww_resampler *r, ww_resample_info *out) {
  WW_GUARD_BEGIN
  if (!r || !out) return ww_fail(r ? r->ctx : nullptr, WW_EINVAL, "ww_resampler_info: NULL argument");
  out->up = r->up;
  out->down = r->down;
  out->half = r->half;
  out->taps_per_output = r->tpp;
  out->table_bytes = (int64_t)r->table_bytes;
  return WW_OK;
  WW_GUARD_END(r ? r->ctx : nullptr)
}

int ww_g711_table(int32_t format, int16_t table[256]) {
  WW_GUARD_BEGIN
  if (!table) return ww_fail(nullptr, WW_EINVAL, "ww_g711_table: NULL table");
  if (format != WW_SAMPLE_MULAW && format != WW_SAMPLE_ALAW)
    return ww_fail(nullptr, WW_EINVAL, "ww_g711_table: format %d: WW_SAMPLE_MULAW or WW_SAMPLE_ALAW", (int)format);
  for (unsigned c = 0; c < 256; ++c) table[c] = (int16_t)(format == WW_SAMPLE_MULAW ? g711_mulaw(c) : g711_alaw(c));
  return WW_OK;
  WW_GUARD_END(nullptr)
}

int ww_resample_dev(ww_resampler *r, const void *d_in, int32_t in_format, const int64_t *sample_offs, const int64_t *in_first,
                    const int64_t *out_first, const int64_t *out_offs, int32_t n_seg, void *d_out, int32_t out_format) {
  WW_GUARD_BEGIN
  if (!r) return ww_fail(nullptr, WW_EINVAL, "ww_resample_dev: NULL resampler");
  ww_ctx *ctx = r->ctx;
  int64_t n_out = 0;
  if (int rc = rs_validate(r, d_in, in_format, sample_offs, in_first, out_first, out_offs, n_seg, d_out, out_format, &n_out)) return rc;
  if (n_out == 0) return WW_OK;
  WW_ON_DEVICE(ctx, dev);
  rs_plan pl;
  rs_make_plan(r, sample_offs, in_first, out_first, out_offs, n_seg, pl);
  if (int rc = ww_ensure(ctx, ctx->dev, ww_bump::need(pl.count(), sizeof(rs_tile)) + 1024, false)) return rc;
  ww_bump bump(ctx->dev.ptr, ctx->dev.cap);
  return rs_run(r, pl, bump.take<rs_tile>(pl.count()), d_in, in_format, d_out, out_format);
  WW_GUARD_END(r ? r->ctx : nullptr)
}

int ww_resample(ww_resampler *r, const void *in, int32_t in_format, const int64_t *sample_offs, const int64_t *in_first,
                const int64_t *out_first, const int64_t *out_offs, int32_t n_seg, void *out, int32_t out_format) {
  WW_GUARD_BEGIN
  if (!r) return ww_fail(nullptr, WW_EINVAL, "ww_resample: NULL resampler");
  ww_ctx *ctx = r->ctx;
  int64_t n_out = 0;
  if (int rc = rs_validate(r, in, in_format, sample_offs, in_first, out_first, out_offs, n_seg, out, out_format, &n_out)) return rc;
  if (n_out == 0) return WW_OK;
  WW_ON_DEVICE(ctx, dev);
  rs_plan pl;
  rs_make_plan(r, sample_offs, in_first, out_first, out_offs, n_seg, pl);
  const size_t ie = rs_sample_bytes(in_format), oe = rs_sample_bytes(out_format);
  const int64_t s0 = sample_offs[0], n_in = sample_offs[n_seg] - s0, o0 = out_offs[0];
  if (int rc = ww_ensure(ctx, ctx->dev, ww_bump::need((size_t)n_in, ie) + ww_bump::need((size_t)n_out, oe) + ww_bump::need(pl.count(), sizeof(rs_tile)) + 1024, false))
    return rc;
  ww_bump bump(ctx->dev.ptr, ctx->dev.cap);
  char *d_in = bump.take<char>((size_t)n_in * ie), *d_out = bump.take<char>((size_t)n_out * oe);
  rs_tile *d_tiles = bump.take<rs_tile>(pl.count());
  if (n_in > 0) WW_HIP(ctx, hipMemcpyAsync(d_in, (const char *)in + s0 * ie, (size_t)n_in * ie, hipMemcpyHostToDevice, ctx->stream));
  // the kernels index the buffers by the caller's offsets: shift the bases instead of the tables
  if (int rc = rs_run(r, pl, d_tiles, d_in - s0 * (int64_t)ie, in_format, d_out - o0 * (int64_t)oe, out_format)) return rc;
  WW_HIP(ctx, hipMemcpyAsync((char *)out + o0 * oe, d_out, (size_t)n_out * oe, hipMemcpyDeviceToHost, ctx->stream));
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return WW_OK;
  WW_GUARD_END(r ? r->ctx : nullptr)
}

}  // extern "C"

// ---- stream banks at other rates than 16 kHz (streams.hip: ww_stream_attach_resampler, ww_stream_attach_rates) --
// The bank's kernels are untouched: ONE kernel in front of a tick turns the S streams' frames, each at its stream's rate (F = rate /
// 50 samples, page-locked), into the [S][320] int16 block the tick kernels read their samples from.  Up to WW_STREAM_MAX_RATES rate
// classes, stream s in class cls[s]; the geometry and the bookkeeping are stream_rate.h's and stream_rates.h's (host only); the
// arithmetic is this file's rule - rs_load, ONE chain per output over the class's own tap table, rs_store -, so a stream's 16 kHz
// samples are the one-shot's bits behind D zeros.  The 16 kHz class has no resampler: its samples pass through.
// ONE state object serves both kinds of bank.  A `uniform` bank (ww_stream_attach_resampler) is the bank of one resampling class
// with every stream in it for good: its frames are [S][F], and no per-stream descriptor is sent or read.  A per-stream bank's
// frames are one ragged block (stream s's frame from sample desc[s].off); the descriptor {class, offset} is a DEVICE table (resent
// when a stream moves), so the frame's first 320 16-byte pieces are requested before anything that crossed the bus is looked at.
// One workgroup per stream, one lane per output.  A stream's state is the last `hist` input samples of its class as fp32
// (right-aligned; of a young stream only the last `held` are its own, what lies in front reads as zero - a reset or a move is the
// host's count = 0, no kernel): read into LDS in front of the frame by the one workgroup that writes it back, no order between
// workgroups.  The history rows are per class, [S][hist of the class], and a stream uses its current class's row only: whatever an
// earlier use left in a row reads as zero behind held = 0, so a move clears nothing.
// Formats (stream_formats.h): a class reads its frames and packets as int16 or as G.711 mu-law / A-law, one byte per
// sample.  Only the unpacking knows: the tick's kernel takes a frame as F x bytes-per-sample bytes from any byte (an int16 frame: any
// even byte) and decodes a G.711 piece's 16 samples where it unpacks an int16 piece's 8, the feed's splice and pass-through copy take
// byte offsets and the class's format.  What is staged is rs_load of the decoded int16 value, so everything behind - chains,
// history, outputs - has the decoded int16 input's bits.
struct ww_stream_rates {
  ww_ctx *ctx = nullptr;
  int S = 0;
  bool uniform = false;  // made by ww_stream_attach_resampler (NOT: K happens to be 1 - a per-stream bank of one class may still be moved)
  rates_table tab;
  formats_table fmt;  // the classes' sample formats (stream_formats.h); all int16 unless the bank was attached with formats
  const ww_resampler *r[WW_STREAM_MAX_RATES] = {};  // the class's resampler, whose tap table the kernels borrow; nullptr: the 16 kHz class
  float *d_hist[WW_STREAM_MAX_RATES] = {};          // [S][hist of the class]
  std::vector<int32_t> cls;                         // [S] the stream's class
  std::vector<int64_t> n;  // [S] input samples since the stream's last reset or move, frozen ticks left out (a 16 kHz stream's stays 0)
  std::vector<rates_desc> desc;                     // [S] what d_desc was last sent
  int64_t total = 0;                                // bytes of a tick's frames
  rates_desc *d_desc = nullptr;                     // (a uniform bank has none)
  int16_t *d_out = nullptr;  // [S][320]: the tick's 16 kHz samples (640 bytes per stream: the tick kernels load them 16 at a time)
  // the tick's page-locked input: [S] rate_ctl | the frames (room for S frames of the longest class).  ONE copy: the kernel that
  // reads it precedes the tick's kernel on the stream, so it has ended when a polled tick's first tag arrives
  char *h_in = nullptr, *h_in_dev = nullptr;
  size_t lds_bytes = 0;
  ww_resampler pass_r;        // the 16 kHz class of a feed: the identity form's tiles (resample_copy_kernel), no table
  char *d_scratch = nullptr;  // a feed's [packets | per class present: splice table | segments | tiles], grown on demand
  size_t scratch_cap = 0;
  void layout() {  // (stream_formats.h: formats_layout)
    total = 0;
    for (int s = 0; s < S; ++s) {
      const int c = cls[(size_t)s], b = format_bytes(fmt.fmt[c]);
      total = formats_frame_start(total, b);
      desc[(size_t)s] = {total, c, 0};
      total += (int64_t)tab.g[c].F * b;
    }
  }
  int send() {
    ww_tables tb;
    tb.add(desc);
    return tb.send(ctx, d_desc);
  }
};

struct rate_class_dev {
  const float *taps;
  float *hist;  // [S][H]
  int up, down, half, tpp, F, D, H, pass;
  int law;  // 0: int16 samples; WW_SAMPLE_MULAW / WW_SAMPLE_ALAW: one byte per sample, decoded as it is unpacked
};
template <int K>
struct rate_tick_args {
  const int16_t *frames;   // page-locked, from a 16-byte boundary, padded to whole 16-byte pieces (a byte block: int16 and G.711 frames)
  const rate_ctl *rc;      // page-locked [S]
  const int32_t *ctl;      // the tick's own control words [S][4] (page-locked): bit 1 of word 2 = the stream is frozen
  int16_t *out;
  rate_class_dev c[K];
  const rates_desc *desc;  // device [S]; a uniform bank: not read (last, so that K = 1 loads its arguments as flat ones would be)
};

#define RATE_THREADS WW_RATE_FRAME_OUT

// PerStream = false, a uniform bank: frame s lies at s * F and the one class's geometry is read from fixed argument slots - nothing
// is loaded in front of the frame.  PerStream = true: the descriptor comes from the device table and picks the class's geometry
// with a wave-uniform index (scalar loads of the arguments); the 16 kHz class copies its frame.
template <bool PerStream>
__global__ __launch_bounds__(RATE_THREADS) void stream_rate_tick_kernel(rate_tick_args<PerStream ? WW_STREAM_MAX_RATES : 1> a) {
  extern __shared__ float xs[];  // [H history | F frame | WW_RATE_PAD zeros] of the stream's class
  const int s = blockIdx.x, tid = threadIdx.x;
  const rate_class_dev *cp = &a.c[0];
  size_t b0;  // the frame's first byte
  if constexpr (PerStream) {
    const rates_desc d = a.desc[s];
    cp = &a.c[__builtin_amdgcn_readfirstlane(d.cls) & (WW_STREAM_MAX_RATES - 1)];
    b0 = (size_t)d.off;  // (the table holds byte offsets: an int16 frame's is even)
  } else {
    b0 = (size_t)s * a.c[0].F * (a.c[0].law ? 1 : 2);
  }
  const rate_class_dev &g = *cp;
  const int F = g.F, H = g.H, law = g.law;  // (law: wave-uniform, like every field of the class)
  // A G.711 class decodes through a 256-entry table in LDS, filled here by 256 lanes with one code each: the few lanes that hold the
  // frame's pieces would else run 16 decodes in a row each (measured: a few tenths of a microsecond per tick at 128 streams).  The entries
  // are rs_load of the decoded int16 values - what the int16 path stages.
  __shared__ float g711_tab[256];
  if (law) {
    if (tid < 256) g711_tab[tid] = rs_load((int16_t)g711_decode(law, (unsigned)tid));
    __syncthreads();  // (the class is the workgroup's: every lane comes here or none does)
  }
  // The frame crosses the bus 16 bytes per lane, whatever F is: the aligned 16-byte pieces that cover its bytes - 2 F of an int16
  // frame, which starts at any even byte, F of a G.711 frame, which starts at any byte (the first and the last piece may hold a
  // neighbour's samples, which are dropped; the block is padded to whole pieces).  The first RATE_THREADS pieces are requested BEFORE
  // the control words are looked at - one trip over the bus instead of two in a row.
  const size_t a0 = b0 & ~(size_t)15;
  const int n16 = (int)((b0 + (size_t)F * (law ? 1 : 2) - a0 + 15) >> 4), lead = law ? (int)(b0 - a0) : (int)(b0 - a0) >> 1;  // lead: samples
  const uint4 *src = (const uint4 *)((const char *)a.frames + a0);
  uint4 raw = make_uint4(0u, 0u, 0u, 0u);
  if (tid < n16) raw = src[tid];
  const int flags = a.ctl[s * 4 + 2];
  const int4 cw = ((const int4 *)a.rc)[s];  // res, zeros, held
  if (flags & 2) return;  // frozen: the frame is dropped whole, history and output block stay
  if constexpr (PerStream) {
    if (g.pass) {  // the 16 kHz class: the frame is the stream's row of the block (41 pieces at most: one per lane)
      int16_t *o = a.out + (size_t)s * WW_RATE_FRAME_OUT;
      const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
      if (law) {  // 16 kHz G.711: the decoded frame is the row (21 pieces at most)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = tid * 16 + e - lead;
          if (tid < n16 && i >= 0 && i < WW_RATE_FRAME_OUT) o[i] = (int16_t)(g711_tab[(w[e >> 2] >> ((e & 3) * 8)) & 0xFFu] * 32768.0f);  // (exact: the entry is the value / 2^15)
        }
        return;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = tid * 8 + e - lead;
        if (tid < n16 && i >= 0 && i < WW_RATE_FRAME_OUT) o[i] = (int16_t)(w[e >> 1] >> ((e & 1) * 16));
      }
      return;
    }
  }
  float *hist = g.hist + (size_t)s * H;
  auto put = [&](int q, const uint4 &v) {  // piece q: samples 8 q - lead .. 8 q - lead + 7 of the frame (G.711: 16 q - lead .. + 15)
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    if (law) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = q * 16 + e - lead;
        if (i >= 0 && i < F) xs[H + i] = g711_tab[(w[e >> 2] >> ((e & 3) * 8)) & 0xFFu];
      }
      return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = q * 8 + e - lead;
      if (i >= 0 && i < F) xs[H + i] = rs_load((int16_t)(w[e >> 1] >> ((e & 1) * 16)));
    }
  };
  if (tid < n16) put(tid, raw);
  for (int q = tid + RATE_THREADS; q < n16; q += RATE_THREADS) put(q, src[q]);
  for (int i = tid; i < H; i += RATE_THREADS) xs[i] = i >= H - cw.z ? hist[i] : 0.0f;
  if (tid < WW_RATE_PAD) xs[H + F + tid] = 0.0f;
  __syncthreads();
  const int up = g.up, down = g.down;
  const rate_out_pos o = rate_position(up, down, g.D, tid, cw.x);
  float acc[1];
  rs_chains<1>(acc, xs + H + o.c - rs_jmax(g.half, o.p, up), g.taps + o.p, up, down, g.tpp);
  rs_store(a.out + (size_t)s * WW_RATE_FRAME_OUT + tid, tid < cw.y ? 0.0f : acc[0]);
  for (int i = tid; i < H; i += RATE_THREADS) hist[i] = xs[F + i];  // (every read of the row went through LDS above)
}

// A feed's splice: stream d.sid's segment = [the `held` samples it holds | its packet of k] as fp32 for the resample kernels, and its
// new history behind their reads.  Workgroup (i, c) copies samples [c * RATE_SPLICE, +RATE_SPLICE) of the segment; history rows
// are shorter than that, so workgroup (i, 0) is the row's one reader, and it is its one writer.
#define RATE_SPLICE 16384
struct rate_feed_str {
  int64_t pk_off;   // the packet's first BYTE in the call's packet buffer (an int16 packet's is even)
  int64_t k;        // its samples (> 0)
  int64_t seg_off;  // the segment's first sample in the class's segment buffer
  int32_t sid, held;
};
__global__ __launch_bounds__(256) void stream_rate_splice_kernel(const char *pk, const rate_feed_str *str, float *seg, float *hist, int H, int law) {
  extern __shared__ float nh[];  // [H]
  const rate_feed_str d = str[blockIdx.x];
  float *h = hist + (size_t)d.sid * H;
  const int64_t tot = d.held + d.k, v0 = (int64_t)blockIdx.y * RATE_SPLICE;
  if (v0 >= tot) return;
  auto sample = [&](int64_t v) -> float {  // (law: the class's format, the same for every packet of the launch)
    if (v < d.held) return h[H - d.held + v];
    if (law) return rs_load((int16_t)g711_decode(law, (unsigned char)pk[d.pk_off + (v - d.held)]));
    return rs_load(((const int16_t *)(pk + d.pk_off))[v - d.held]);
  };
  const int64_t v1 = v0 + RATE_SPLICE < tot ? v0 + RATE_SPLICE : tot;
  for (int64_t v = v0 + threadIdx.x; v < v1; v += 256) seg[d.seg_off + v] = sample(v);
  if (blockIdx.y) return;
  const int keep = (int)(tot < H ? tot : H);
  for (int i = threadIdx.x; i < keep; i += 256) nh[i] = sample(tot - keep + i);
  __syncthreads();  // the row has been read
  for (int i = threadIdx.x; i < keep; i += 256) h[H - keep + i] = nh[i];
}

void ww_k_rates_destroy(ww_stream_rates *rt) {
  if (!rt) return;
  for (float *h : rt->d_hist)
    if (h) hipFree(h);
  if (rt->d_desc) hipFree(rt->d_desc);
  if (rt->d_out) hipFree(rt->d_out);
  if (rt->d_scratch) hipFree(rt->d_scratch);
  if (rt->h_in) hipHostFree(rt->h_in);
  delete rt;
}

static int rates_destroy_(ww_stream_rates *rt) {
  ww_k_rates_destroy(rt);
  return WW_OK;
}

int ww_k_rates_create(ww_ctx *ctx, const ww_resampler *const *rs, const int32_t *formats, int n_rates, const int32_t *stream_rate, int S, bool uniform,
                      const char *what, ww_stream_rates **out) {
  *out = nullptr;
  char why[320];
  ww_stream_rates *rt = new ww_stream_rates();
  ww_scoped<ww_stream_rates, rates_destroy_> own(rt);
  rt->ctx = ctx; rt->S = S; rt->uniform = uniform;
  rt->pass_r.ctx = ctx;
  rt->pass_r.identity = true;
  rt->pass_r.rate_in = rt->pass_r.rate_out = WW_RATE_OUT;
  if (uniform) {  // the one class on its own: rate_make_geom's refusals, no class named
    const ww_resampler *r = rs[0];
    if (r->ctx != ctx) return ww_fail(ctx, WW_EINVAL, "%s: the resampler belongs to another context", what);
    if (formats && !format_bytes(formats[0]))
      return ww_fail(ctx, WW_EINVAL, "%s: format %d: a bank reads WW_SAMPLE_I16, WW_SAMPLE_MULAW or WW_SAMPLE_ALAW (float32 streams are not offered)", what,
                     (int)formats[0]);
    if (rate_make_geom(r->rate_in, r->rate_out, r->up, r->down, r->half, r->tpp, rt->tab.g[0], why, sizeof why))
      return ww_fail(ctx, WW_EINVAL, "%s: %s", what, why);
    rt->tab.K = 1;
    if (formats) {
      rt->fmt.fmt[0] = formats[0];
      rt->fmt.g711 = format_bytes(formats[0]) == 1;
    }
  } else if (formats) {  // classes are (rate, format) pairs (stream_formats.h)
    for (int k = 0; k < n_rates; ++k) {
      const ww_resampler *r = rs[k];
      if (r && r->ctx != ctx) return ww_fail(ctx, WW_EINVAL, "%s: class %d: the resampler belongs to another context", what, k);
      if (r ? formats_add_class(rt->tab, rt->fmt, formats[k], false, r->rate_in, r->rate_out, r->up, r->down, r->half, r->tpp, why, sizeof why)
            : formats_add_class(rt->tab, rt->fmt, formats[k], true, 0, 0, 0, 0, 0, 0, why, sizeof why))
        return ww_fail(ctx, WW_EINVAL, "%s: %s", what, why);
    }
  } else {
    for (int k = 0; k < n_rates; ++k) {
      const ww_resampler *r = rs[k];
      if (r && r->ctx != ctx) return ww_fail(ctx, WW_EINVAL, "ww_stream_attach_rates: class %d: the resampler belongs to another context", k);
      if (r ? rates_add_class(rt->tab, false, r->rate_in, r->rate_out, r->up, r->down, r->half, r->tpp, why, sizeof why)
            : rates_add_class(rt->tab, true, 0, 0, 0, 0, 0, 0, why, sizeof why))
        return ww_fail(ctx, WW_EINVAL, "ww_stream_attach_rates: %s", why);
    }
  }
  if (rates_check_ids(rt->tab, stream_rate, S, "stream_rate", why, sizeof why)) return ww_fail(ctx, WW_EINVAL, "%s: %s", what, why);
  int64_t stage = 0;
  if (rates_stage(rt->tab, &stage, why, sizeof why)) return ww_fail(ctx, WW_EINVAL, "%s: %s", what, why);
  rt->lds_bytes = (size_t)stage * 4;
  if (stream_rate) rt->cls.assign(stream_rate, stream_rate + S);
  else rt->cls.assign((size_t)S, 0);
  rt->n.assign((size_t)S, 0);
  rt->desc.resize((size_t)S);
  rt->layout();
  // (the frames start on a 16-byte boundary and end in whole 16-byte pieces: the kernel loads them as uint4)
  const size_t b_desc = ww_bump::need((size_t)S, sizeof(rates_desc)), b_out = (size_t)S * WW_RATE_FRAME_OUT * 2,
               b_in = (size_t)S * sizeof(rate_ctl) + (((size_t)formats_layout_max(rt->tab, rt->fmt, S) + 15) & ~(size_t)15) + 16;
  bool ok = hipMalloc((void **)&rt->d_out, b_out) == hipSuccess && hipHostMalloc((void **)&rt->h_in, b_in) == hipSuccess &&
            (uniform || hipMalloc((void **)&rt->d_desc, b_desc) == hipSuccess);
  for (int k = 0; k < n_rates && ok; ++k) {
    rt->r[k] = rs[k];
    if (rs[k]) ok = hipMalloc((void **)&rt->d_hist[k], (size_t)S * rt->tab.g[k].hist * 4) == hipSuccess;
  }
  if (!ok)
    return uniform ? ww_fail(ctx, WW_ENOMEM, "cannot allocate the resampling state of %d streams at %d Hz", S, rt->tab.g[0].rate_in)
                   : ww_fail(ctx, WW_ENOMEM, "cannot allocate the rate tables of %d streams in %d classes", S, n_rates);
  if (((uintptr_t)rt->d_out & 15) != 0) return ww_fail(ctx, WW_EINTERNAL, "the tick's sample block is not 16-byte aligned");
  memset(rt->h_in, 0, b_in);
  WW_HIP(ctx, hipHostGetDevicePointer((void **)&rt->h_in_dev, rt->h_in, 0));
  for (int k = 0; k < n_rates; ++k)
    if (rs[k]) WW_HIP(ctx, hipMemsetAsync(rt->d_hist[k], 0, (size_t)S * rt->tab.g[k].hist * 4, ctx->stream));
  WW_HIP(ctx, hipMemsetAsync(rt->d_out, 0, b_out, ctx->stream));
  if (!uniform)
    if (int rc = rt->send()) return rc;
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *out = own.release();
  return WW_OK;
}

int ww_k_rates_classes(const ww_stream_rates *rt) { return rt->tab.K; }

int ww_k_rates_frame_samples(const ww_stream_rates *rt) { return rt->uniform ? rt->tab.g[0].F : 0; }

bool ww_k_rates_g711(const ww_stream_rates *rt) { return rt->fmt.g711; }

int ww_k_rates_stream_format(const ww_stream_rates *rt, int stream) { return rt->fmt.fmt[rt->cls[(size_t)stream]]; }

void ww_k_rates_layout_bytes(const ww_stream_rates *rt, int32_t *frame_bytes, int64_t *byte_offs, int32_t *formats) {
  formats_layout(rt->tab, rt->fmt, rt->cls.data(), rt->S, frame_bytes, byte_offs, formats);
}

void ww_k_rates_layout(const ww_stream_rates *rt, int32_t *frame_samples, int64_t *frame_offs) {
  rates_layout(rt->tab, rt->cls.data(), rt->S, frame_samples, frame_offs);
}

void ww_k_rates_reset(ww_stream_rates *rt, const int32_t *ids, int count) {
  for (int i = 0; i < count; ++i) {
    const int s = ids ? ids[i] : i;
    rates_move(rt->cls[(size_t)s], rt->n[(size_t)s], rt->cls[(size_t)s]);  // the next sample is x[0] of a new signal: D zeros lead again
  }
}

// The listed streams move to class c (checked by the caller) with their counts at 0, and the table goes up in stream order.  A
// failure leaves the host's table as the device's was last sent; the caller marks the bank broken (the copy may have been enqueued).
int ww_k_rates_move(ww_stream_rates *rt, const int32_t *ids, int count, int c) {
  const std::vector<int32_t> before = rt->cls;
  for (int i = 0; i < count; ++i) {
    const int s = ids ? ids[i] : i;
    rates_move(rt->cls[(size_t)s], rt->n[(size_t)s], c);
  }
  rt->layout();
  if (int rc = rt->send()) {
    rt->cls = before;
    rt->layout();
    return rc;
  }
  return WW_OK;
}

int64_t ww_k_rates_advance(const ww_stream_rates *rt, int stream, int64_t k) {
  return rates_advance(rt->tab, rt->cls[(size_t)stream], rt->n[(size_t)stream], k);
}

template <int K>
static void rates_tick_launch(const ww_stream_rates *rt, const int32_t *ctl_dev) {
  rate_tick_args<K> a = {};
  a.rc = (const rate_ctl *)rt->h_in_dev;
  a.frames = (const int16_t *)(rt->h_in_dev + (size_t)rt->S * sizeof(rate_ctl));
  a.ctl = ctl_dev;
  a.desc = rt->d_desc;
  a.out = rt->d_out;
  for (int k = 0; k < K; ++k) {
    const int j = k < rt->tab.K ? k : 0;  // (a slot above the bank's classes is never picked: a class id is below tab.K)
    const rate_geom &g = rt->tab.g[j];
    a.c[k] = {rt->r[j] ? rt->r[j]->d_taps : nullptr, rt->d_hist[j], (int)g.up, (int)g.down, (int)g.half, (int)g.tpp, g.F, g.D, g.hist, rt->tab.pass[j] ? 1 : 0,
              format_bytes(rt->fmt.fmt[j]) == 1 ? rt->fmt.fmt[j] : 0};
  }
  ww_launch_scope scope(rt->ctx, K == 1 ? "stream_rate_tick_kernel" : "stream_rates_tick_kernel");
  hipLaunchKernelGGL((stream_rate_tick_kernel<(K > 1)>), dim3((unsigned)rt->S), dim3(RATE_THREADS), rt->lds_bytes, rt->ctx->stream, a);
}

int ww_k_rates_tick(ww_stream_rates *rt, const int16_t *frames, const uint8_t *flags, const int32_t *ctl_dev, const int16_t **d_frames) {
  ww_ctx *ctx = rt->ctx;
  const int S = rt->S;
  rate_ctl *rc = (rate_ctl *)rt->h_in;
  for (int s = 0; s < S; ++s) {
    if (flags[s] & 2) continue;
    rc[s] = rates_tick(rt->tab, rt->cls[(size_t)s], rt->n[(size_t)s]);
  }
  memcpy(rt->h_in + (size_t)S * sizeof(rate_ctl), frames, (size_t)rt->total);
  if (rt->uniform) rates_tick_launch<1>(rt, ctl_dev);
  else rates_tick_launch<WW_STREAM_MAX_RATES>(rt, ctl_dev);
  WW_HIP(ctx, hipGetLastError());
  *d_frames = rt->d_out;
  return WW_OK;
}

// A feed's packets, stream ids[i]'s at its own rate -> the call's 16 kHz samples at d_dst[offs16[i] .. offs16[i + 1]), offs16 as
// ww_k_rates_advance counts them.  The packets go up once and are grouped by class (stream_rates.h; a uniform bank has one group
// that holds every packet): the 16 kHz class's go to their place through the identity form's tiles, every other class's through
// the splice and the class's own resample kernels - launches and copies per class present, whatever the number of streams.
// Everything a refusal depends on is planned before any state moves.  *moved: sample counts have advanced (a failure behind that
// point leaves the bank's host mirrors and its device state out of step).
struct rate_feed_class {
  std::vector<rate_feed_str> str;  // the splice's packets (a resampling class)
  rs_plan pl;
  int64_t seg_total = 0, k_max = 0;
};

int ww_k_rates_feed(ww_stream_rates *rt, const int32_t *ids, int n, const void *data, const int64_t *byte_offs, const int64_t *offs16,
                    int16_t *d_dst, bool *moved) {
  ww_ctx *ctx = rt->ctx;
  const int K = rt->tab.K;
  std::vector<int32_t> pc((size_t)n);
  for (int i = 0; i < n; ++i) pc[(size_t)i] = rt->cls[(size_t)ids[i]];
  rates_groups grp;
  rates_group(pc.data(), n, grp);
  // packet i is bytes [byte_offs[i], byte_offs[i + 1]) of `data` in its class's format (the caller has checked int16 packets for
  // even offsets and lengths); the upload starts at an even byte, so an int16 packet is as aligned on the device as on the host
  const int64_t s0 = byte_offs[0] & ~(int64_t)1, bytes = byte_offs[n] - s0;
  rate_feed_class work[WW_STREAM_MAX_RATES];
  size_t need = ww_bump::need((size_t)bytes, 1) + 1024;
  for (int c = 0; c < K; ++c) {
    rate_feed_class &w = work[c];
    const int bps = format_bytes(rt->fmt.fmt[c]);
    for (int j = grp.start[c]; j < grp.start[c + 1]; ++j) {
      const int i = grp.order[(size_t)j], s = ids[i];
      const int64_t k = (byte_offs[i + 1] - byte_offs[i]) / bps, p0 = byte_offs[i] - s0;  // the packet's samples | its first byte of the upload
      if (k == 0) continue;
      if (!rt->r[c]) {  // (the identity form's tiles count samples of the class's format from the upload's start)
        const int64_t so[2] = {p0 / bps, p0 / bps + k}, first[1] = {0}, oo[2] = {offs16[i], offs16[i + 1]};
        rs_make_plan(&rt->pass_r, so, first, first, oo, 1, w.pl);
        continue;
      }
      const rate_step st = rate_advance(rt->tab.g[c], rt->n[(size_t)s], k);
      w.str.push_back({p0, k, w.seg_total, s, st.held});
      if (st.count > st.zeros) {
        // the segment's first sample is input n - held of the stream; its outputs land behind the zeros of the stream's 16 kHz run
        const int64_t so[2] = {w.seg_total, w.seg_total + st.held + k}, in_first[1] = {rt->n[(size_t)s] - st.held}, out_first[1] = {st.y0},
                      oo[2] = {offs16[i] + st.zeros, offs16[i + 1]};
        rs_make_plan(rt->r[c], so, in_first, out_first, oo, 1, w.pl);
      }
      w.seg_total += st.held + k;
      w.k_max = std::max(w.k_max, st.held + k);
    }
    if (w.str.size() > 0x7fffffffu || w.pl.count() > 0x7fffffffu || (w.k_max + RATE_SPLICE - 1) / RATE_SPLICE > 65535)
      return ww_fail(ctx, WW_EINVAL, "ww_stream_feed: too much work for one call");
    need += ww_bump::need(w.str.size(), sizeof(rate_feed_str)) + ww_bump::need((size_t)w.seg_total, 4) + ww_bump::need(w.pl.count(), sizeof(rs_tile));
  }
  if (need > rt->scratch_cap) {
    WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (rt->d_scratch) WW_HIP(ctx, hipFree(rt->d_scratch));
    rt->d_scratch = nullptr;
    rt->scratch_cap = 0;
    if (hipMalloc((void **)&rt->d_scratch, need) != hipSuccess)
      return rt->uniform ? ww_fail(ctx, WW_ENOMEM, "ww_stream_feed: cannot allocate %zu bytes for the call's samples at %d Hz", need, rt->tab.g[0].rate_in)
                         : ww_fail(ctx, WW_ENOMEM, "ww_stream_feed: cannot allocate %zu bytes for the call's samples", need);
    rt->scratch_cap = need;
  }
  ww_bump db(rt->d_scratch, rt->scratch_cap);
  char *d_pk = db.take<char>((size_t)bytes);
  WW_HIP(ctx, hipMemcpyAsync(d_pk, (const char *)data + s0, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
  if (offs16[n] > 0) WW_HIP(ctx, hipMemsetAsync(d_dst, 0, (size_t)offs16[n] * 2, ctx->stream));  // z's leading zeros
  // (each class has its own region of the scratch: a class's table goes up now, its kernels run later on the stream)
  for (int c = 0; c < K; ++c) {
    const rate_feed_class &w = work[c];
    if (grp.start[c + 1] == grp.start[c]) continue;
    rate_feed_str *d_str = db.take<rate_feed_str>(w.str.size());
    float *d_seg = db.take<float>((size_t)w.seg_total);
    rs_tile *d_tiles = db.take<rs_tile>(w.pl.count());
    if (!rt->r[c]) {
      if (w.pl.count() > 0)
        if (int rc = rs_run(&rt->pass_r, w.pl, d_tiles, d_pk, rt->fmt.fmt[c], d_dst, WW_SAMPLE_I16)) return rc;
      continue;
    }
    *moved = true;
    for (const rate_feed_str &d : w.str) rt->n[(size_t)d.sid] += d.k;
    if (w.str.empty()) continue;
    ww_tables tb;
    tb.add(w.str);
    if (int rc = tb.send(ctx, d_str)) return rc;
    {
      ww_launch_scope scope(ctx, "stream_rate_splice_kernel");
      hipLaunchKernelGGL(stream_rate_splice_kernel, dim3((unsigned)w.str.size(), (unsigned)((w.k_max + RATE_SPLICE - 1) / RATE_SPLICE)), dim3(256),
                         (size_t)rt->tab.g[c].hist * 4, ctx->stream, (const char *)d_pk, (const rate_feed_str *)d_str, d_seg, rt->d_hist[c],
                         (int)rt->tab.g[c].hist, format_bytes(rt->fmt.fmt[c]) == 1 ? (int)rt->fmt.fmt[c] : 0);
    }
    WW_HIP(ctx, hipGetLastError());
    if (w.pl.count() > 0)
      if (int rc = rs_run(rt->r[c], w.pl, d_tiles, d_seg, WW_SAMPLE_F32, d_dst, WW_SAMPLE_I16)) return rc;
  }
  return WW_OK;
}

