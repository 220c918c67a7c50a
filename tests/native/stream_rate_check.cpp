// stream_rate_check - csrc/stream_rate.h (the host-only geometry of a stream bank at another rate than 16 kHz) alone on the CPU,
// under Address + UB sanitizer (tests/test_stream_rate_host.py compiles and runs it; nothing here touches a GPU).  For every
// standard rate and for a non-default filter (zeros = 8):
//   * F, D, taps per output and the history length - against the table of DESIGN.md 7.4 for the default filter;
//   * over random packet cuts mixed with ticks: the outputs of the calls sum to floor(N * up / down), z's zeros and y's indices
//     follow one another without gap, every emitted output is determined by the samples that have arrived, and its first input is
//     still in the stream's history;
//   * for every residue a stream can be at and every output of a tick: rate_position's (c, p) are the output's first input and
//     phase as the absolute indices give them, and the chain's reads stay inside [history | frame | pad];
//   * the refusals: 11025 Hz, 16000 Hz, an output rate other than 16000 Hz, a geometry too long for a tick's staging;
//   * the staging cap from both sides: all of the above at 500000 Hz (12,156 of 12,288 staged floats), and 510000 Hz refused.
// Prints one "geom <zeros> <rate> <up> <down> <half> <F> <D> <history>" line per geometry and then "ok <checks>" and exits 0, or says
// what failed and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "stream_rate.h"

static long n_checks = 0;
#define CHECK(cond)                                                                                       \
  do {                                                                                                    \
    ++n_checks;                                                                                           \
    if (!(cond)) {                                                                                        \
      fprintf(stderr, "stream_rate_check: %s (line %d, rate %d)\n", #cond, __LINE__, (int)cur_rate);     \
      exit(1);                                                                                            \
    }                                                                                                     \
  } while (0)
static int cur_rate = 0;

// the filter's length as ww_resampler_create and wwhip.resample.design state it
static void design(int rate_in, int zeros, double rolloff, int64_t &up, int64_t &down, int64_t &half, int64_t &tpp) {
  const int64_t g = std::gcd((int64_t)rate_in, (int64_t)16000);
  up = 16000 / g;
  down = rate_in / g;
  const double L = (double)((int64_t)rate_in * up), f2 = rolloff * (double)(rate_in < 16000 ? rate_in : 16000) / L;
  half = (int64_t)std::ceil((double)zeros / f2);
  tpp = (2 * half + 1 + up - 1) / up;
}

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)((rng_state >> 33) % n);
}

static int64_t mod(int64_t a, int64_t b) { return ((a % b) + b) % b; }

static void check_rate(int rate_in, int zeros, const int *table /* up, down, half, F, D, tpp or nullptr */) {
  cur_rate = rate_in;
  int64_t up, down, half, tpp;
  design(rate_in, zeros, 0.945, up, down, half, tpp);
  rate_geom g;
  char why[256] = {0};
  CHECK(rate_make_geom(rate_in, 16000, up, down, half, tpp, g, why, sizeof why) == 0);
  // (for tests/test_stream_rate_host.py, which holds these against wwhip.resample's own arithmetic)
  printf("geom %d %d %lld %lld %lld %d %d %d\n", zeros, rate_in, (long long)up, (long long)down, (long long)half, g.F, g.D, g.hist);
  if (table) {
    CHECK(up == table[0] && down == table[1] && half == table[2]);
    CHECK(g.F == table[3] && g.D == table[4] && tpp == table[5]);
  }
  CHECK(g.F * 50 == rate_in && (int64_t)g.F * up == 320 * down);
  CHECK(g.D == (half + down - 1) / down && half < down * (g.D + 1));
  const int64_t aligned = (g.D * down + half + up - 1) / up + 1;
  CHECK(g.hist >= aligned && g.hist >= ((g.D + 1) * down + half + up - 1) / up && g.hist <= aligned + down);
  if (zeros == 32 && rate_in <= 192000) CHECK(aligned <= 816 && g.hist <= 828);  // (the standard rates' histories)
  CHECK(g.hist + g.F + WW_RATE_PAD <= WW_RATE_STAGE_MAX);

  // ---- random cuts: packets of 1 .. 3000 samples, empty packets and ticks of F, from a reset
  for (int trial = 0; trial < 6; ++trial) {
    int64_t n = 0, total = 0, next_z = 0, next_y = 0;
    for (int call = 0; call < 200; ++call) {
      const unsigned kind = rnd(8);
      const int64_t k = kind == 0 ? g.F : kind == 1 ? 0 : kind == 2 ? 1 + rnd(7) : 1 + rnd(3000);
      const rate_step st = rate_advance(g, n, k);
      CHECK(st.z0 == next_z && st.count >= 0 && st.zeros >= 0 && st.zeros <= st.count);
      CHECK(st.z0 == (int64_t)(((__int128)n * up) / down));
      CHECK(st.res == (int64_t)(((__int128)n * up) % down) && st.held == (n < g.hist ? n : g.hist));
      if (k == g.F) CHECK(st.count == 320);
      for (int64_t j = 0; j < st.zeros; ++j) CHECK(st.z0 + j < g.D);
      if (st.count > st.zeros) {
        CHECK(st.y0 == next_y && st.y0 == st.z0 + st.zeros - g.D && st.y0 >= 0);
        const int64_t y_last = st.y0 + (st.count - st.zeros) - 1;
        CHECK(rate_last_input(g, y_last) <= n + k - 1);                  // determined by what has arrived
        CHECK(rate_first_input(g, st.y0) >= n - g.hist);                 // and its first input is still held (or lies in front of x[0])
        next_y = y_last + 1;
      }
      next_z += st.count;
      total += st.count;
      n += k;
      CHECK(total == (int64_t)(((__int128)n * up) / down));
    }
  }

  // ---- a tick at every residue a stream can be at (n * up mod down runs through the multiples of gcd(up, down) = 1)
  std::vector<int64_t> ns;
  for (int64_t r = 0; r < down && r < 64; ++r) ns.push_back(r);                  // young streams: n = 0 .. 63
  for (int64_t r = 0; r < down; r += (down > 97 ? down / 97 : 1)) ns.push_back(5 * (int64_t)g.F + r);
  ns.push_back(7 * (int64_t)g.F + down - 1);
  for (const int64_t n : ns) {
    const rate_step st = rate_advance(g, n, g.F);
    CHECK(st.count == 320);
    for (int j = 0; j < 320; ++j) {
      const rate_out_pos o = rate_position((int)up, (int)down, g.D, j, st.res);
      const int64_t m = st.z0 + j - g.D;  // y's index (negative: one of z's zeros, computed and discarded)
      CHECK(o.p >= 0 && o.p < up && o.p == mod(m * down, up));
      const int64_t jmax = (half - o.p) / up, first = o.c - jmax;  // the chain's first read, input 0 = the frame's first sample
      CHECK(n + first == rate_first_input(g, m));
      CHECK(first >= -(int64_t)g.hist);
      CHECK(first + tpp - 1 <= g.F - 1 + WW_RATE_PAD);
      CHECK(n + first + tpp - 1 >= rate_last_input(g, m));  // the chain covers the output's span
      if (j >= st.zeros) CHECK(m >= 0 && rate_last_input(g, m) <= n + g.F - 1);
      else CHECK(m < 0);
    }
  }
}

int main() {
  // rate_in, up, down, half, F, D, taps per output: DESIGN.md 7.4's table (default filter: zeros = 32, rolloff = 0.945)
  static const int table[][7] = {{8000, 2, 1, 68, 160, 68, 69},        {22050, 320, 441, 14934, 441, 34, 94}, {24000, 2, 3, 102, 480, 34, 103},
                                 {32000, 1, 2, 68, 640, 34, 137},     {44100, 160, 441, 14934, 882, 34, 187}, {48000, 1, 3, 102, 960, 34, 205}};
  for (const auto &row : table) check_rate(row[0], 32, row + 1);
  for (int rate : {88200, 96000, 176400, 192000}) {
    check_rate(rate, 32, nullptr);
    int64_t up, down, half, tpp;
    design(rate, 32, 0.945, up, down, half, tpp);
    rate_geom g;
    char why[256];
    CHECK(rate_make_geom(rate, 16000, up, down, half, tpp, g, why, sizeof why) == 0 && g.D == 34 && tpp >= 374 && tpp <= 815);
  }
  for (int rate : {8000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 12000, 16050}) check_rate(rate, 8, nullptr);
  {  // the staging cap decides what a bank accepts: 500000 Hz fills 12,156 of the 12,288 staged floats, 510000 Hz would need 12,399
    static const int near_cap[6] = {4, 125, 4233, 10000, 34, 2117};
    check_rate(500000, 32, near_cap);
    int64_t up, down, half, tpp;
    design(500000, 32, 0.945, up, down, half, tpp);
    rate_geom g;
    char why[256] = {0};
    CHECK(rate_make_geom(500000, 16000, up, down, half, tpp, g, why, sizeof why) == 0 && g.hist == 2152);
    CHECK(g.hist + g.F + WW_RATE_PAD == 12156 && WW_RATE_STAGE_MAX == 12288);
    CHECK((2 * g.F + 15) / 16 == 1250);  // 16-byte pieces of an aligned int16 frame: four trips of the tick's piece loop (320 lanes)
    design(510000, 32, 0.945, up, down, half, tpp);
    cur_rate = 510000;
    CHECK(up == 8 && down == 255 && rate_refusal(510000, 16000, why, sizeof why) == 0);
    CHECK(rate_make_geom(510000, 16000, up, down, half, tpp, g, why, sizeof why) == 1 && strstr(why, "12399 staged") && strstr(why, "12288"));
  }

  // ---- the refusals, each with its reason
  cur_rate = 0;
  rate_geom g;
  char why[256] = {0};
  CHECK(rate_refusal(11025, 16000, why, sizeof why) == 1 && strstr(why, "220.5") && strstr(why, "fractional"));
  CHECK(rate_refusal(16000, 16000, why, sizeof why) == 1 && strstr(why, "plain bank"));
  CHECK(rate_refusal(48000, 8000, why, sizeof why) == 1 && strstr(why, "output rate"));
  CHECK(rate_refusal(16000, 48000, why, sizeof why) == 1 && strstr(why, "output rate"));
  CHECK(rate_refusal(0, 16000, why, sizeof why) == 1 && rate_refusal(-50, 16000, why, sizeof why) == 1);
  CHECK(rate_refusal(48000, 16000, why, sizeof why) == 0 && rate_refusal(8000, 16000, why, sizeof why) == 0);
  CHECK(rate_make_geom(11025, 16000, 640, 441, 14934, 47, g, why, sizeof why) == 1);
  CHECK(rate_make_geom(48000, 16000, 1, 2, 68, 137, g, why, sizeof why) == 1);   // not this pair's ratio
  CHECK(rate_make_geom(50, 16000, 320, 1, 10837, 68, g, why, sizeof why) == 0 && g.F == 1);  // short frames are fine; long histories are not:
  CHECK(rate_make_geom(384000, 16000, 1, 24, 24 * 600, 24 * 1200 + 1, g, why, sizeof why) == 1 && strstr(why, "staged"));
  printf("ok %ld\n", n_checks);
  return 0;
}
