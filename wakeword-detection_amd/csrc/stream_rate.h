// stream_rate.h - the host-only geometry of a stream bank that runs at another rate than the models' 16 kHz (include/wwhip.h:
// ww_stream_attach_resampler).  Plain C++ like launch_plan.h (no HIP header, no HIP call): common.h includes it for
// the .hip files, and tests/native/stream_rate_check.cpp compiles it alone under Address + UB sanitizer on the CPU.
//
// A resampler (up, down, half) from rate_in to 16 kHz gives y[m] = sum_k h[m * down - k * up] * x[k], |m * down - k * up| <= half.
// The bank's 16 kHz signal is z[n] = 0 (n < D), y[n - D] (n >= D) with D = ceil(half / down): after N input samples the bank has
// consumed floor(N * up / down) samples of z, and every one of them is determined by the N samples (half < down * (D + 1)).
#pragma once

#include <cstdint>
#include <cstdio>

#ifdef __HIPCC__
#define WW_RATE_HD __host__ __device__  // the tick's kernel places its outputs with the functions the CPU check runs
#else
#define WW_RATE_HD
#endif

#define WW_RATE_OUT 16000        // the models' rate
#define WW_RATE_TICKS 50         // ticks per second: a frame is rate / 50 samples (20 ms)
#define WW_RATE_FRAME_OUT 320    // WW_RATE_OUT / WW_RATE_TICKS (= WW_CHUNK)
#define WW_RATE_STAGE_MAX 12288  // floats of [history | frame | pad] a tick's workgroup stages in LDS (48 KB)
#define WW_RATE_PAD 4            // staged zeros behind the frame: a chain's padding taps (stored as +0) reach one sample past it

struct rate_geom {
  int64_t up = 1, down = 1, half = 0, tpp = 0;
  int32_t rate_in = 0;
  int32_t F = 0;     // input samples per tick
  int32_t D = 0;     // zeros in front of z
  int32_t hist = 0;  // input samples a stream keeps between calls
};

static inline int64_t rate_floor_div(int64_t a, int64_t b) {  // b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
static inline int64_t rate_ceil_div(int64_t a, int64_t b) { return -rate_floor_div(-a, b); }

// Can a resampler rate_in -> rate_out not be attached to a bank?  1 and the reason in `why` (for ww_last_error), or 0.
static inline int rate_refusal(int32_t rate_in, int32_t rate_out, char *why, size_t cap) {
  if (rate_out != WW_RATE_OUT) {
    snprintf(why, cap, "the resampler's output rate is %d Hz: a bank's models read %d Hz", rate_out, WW_RATE_OUT);
    return 1;
  }
  if (rate_in == WW_RATE_OUT) {
    snprintf(why, cap, "a resampler from %d Hz to %d Hz: that is a plain bank, nothing to attach", rate_in, WW_RATE_OUT);
    return 1;
  }
  if (rate_in <= 0 || rate_in % WW_RATE_TICKS != 0) {
    snprintf(why, cap, "%d Hz has no whole number of samples in a 20 ms frame (%.1f): rates with a fractional frame are not offered in the tick",
             rate_in, (double)rate_in / WW_RATE_TICKS);
    return 1;
  }
  return 0;
}

// (up, down, half, tpp) are the resampler's (ww_resampler_info).  The history covers a stream at ANY sample count N, not only at a
// tick's multiple of F: the next output's first input lies floor((r + D * down + half) / up) samples back, r = N * up mod down < down;
// never less than the tick-aligned statement ceil((D * down + half) / up) + 1.
static inline int rate_make_geom(int32_t rate_in, int32_t rate_out, int64_t up, int64_t down, int64_t half, int64_t tpp, rate_geom &g, char *why,
                                 size_t cap) {
  if (rate_refusal(rate_in, rate_out, why, cap)) return 1;
  if (up <= 0 || down <= 0 || half <= 0 || up * rate_in != down * (int64_t)rate_out) {
    snprintf(why, cap, "a resampler %d -> %d with up = %lld, down = %lld, half = %lld", rate_in, rate_out, (long long)up, (long long)down, (long long)half);
    return 1;
  }
  g.up = up; g.down = down; g.half = half; g.tpp = tpp;
  g.rate_in = rate_in;
  g.F = rate_in / WW_RATE_TICKS;
  const int64_t D = rate_ceil_div(half, down);
  const int64_t aligned = rate_ceil_div(D * down + half, up) + 1, any = rate_ceil_div((D + 1) * down + half, up);
  const int64_t hist = aligned > any ? aligned : any;
  if (hist + g.F + WW_RATE_PAD > WW_RATE_STAGE_MAX) {
    snprintf(why, cap, "%d Hz needs %lld staged samples per tick (history %lld + frame %d); the tick stages %d at most", rate_in,
             (long long)(hist + g.F + WW_RATE_PAD), (long long)hist, g.F, WW_RATE_STAGE_MAX);
    return 1;
  }
  g.D = (int32_t)D;
  g.hist = (int32_t)hist;
  return 0;
}

// samples of z a stream has consumed after n inputs
static inline int64_t rate_consumed(const rate_geom &g, int64_t n) { return (int64_t)(((__int128)n * g.up) / g.down); }

// What a stream with n inputs so far does with k new ones: it advances by `count` samples of z, z[z0 .. z0 + count), of which the
// first `zeros` are z's leading zeros and the rest y[y0 .. y0 + count - zeros); `res` = n * up mod down, the distance (on the common
// grid) of input n behind output z0's centre line, and `held` = the inputs in front of n that the stream still holds.
struct rate_step {
  int64_t z0, count, zeros, y0;
  int32_t res, held;
};
static inline rate_step rate_advance(const rate_geom &g, int64_t n, int64_t k) {
  rate_step s;
  s.z0 = rate_consumed(g, n);
  s.count = rate_consumed(g, n + k) - s.z0;
  s.zeros = g.D - s.z0;
  s.zeros = s.zeros < 0 ? 0 : s.zeros > s.count ? s.count : s.zeros;
  s.y0 = s.z0 + s.zeros - g.D;
  s.res = (int32_t)(((__int128)n * g.up) % g.down);
  s.held = (int32_t)(n < g.hist ? n : g.hist);
  return s;
}

// first and last input sample (absolute, the first unclamped) that output y[m] reads
static inline int64_t rate_first_input(const rate_geom &g, int64_t m) { return rate_ceil_div(m * g.down - g.half, g.up); }
static inline int64_t rate_last_input(const rate_geom &g, int64_t m) { return rate_floor_div(m * g.down + g.half, g.up); }

// The tick's per-stream control words (page-locked, one int4 per stream): all a workgroup needs besides the geometry
struct rate_ctl {
  int32_t res;    // rate_step::res
  int32_t zeros;  // leading outputs of the tick that are z's zeros
  int32_t held;   // valid samples at the end of the stream's history row (older ones read as zero)
  int32_t pad;
};

// Output j of a tick (z[z0 + j]) in the tick's own coordinates, input 0 = the frame's first sample: v = (j - D) * down - res is the
// output's position on the common grid, c = floor(v / up) the input at or in front of it, p = v - c * up its phase
// (32-bit: |v| < (D + 320) * down + down, far below 2^31 for every geometry rate_make_geom accepts)
struct rate_out_pos {
  int32_t c, p;
};
WW_RATE_HD static inline rate_out_pos rate_position(int up, int down, int D, int j, int res) {
  const int v = (j - D) * down - res;
  rate_out_pos o;
  o.c = v >= 0 ? v / up : -((-v + up - 1) / up);
  o.p = v - o.c * up;
  return o;
}
