// stream_rates_check - csrc/stream_rates.h (the host-only geometry of a stream bank whose streams each run at their own rate) alone
// on the CPU, under Address + UB sanitizer (tests/test_stream_rates_host.py compiles and runs it; nothing here touches a GPU):
//   * the class table: a class's geometry is rate_make_geom's, the 16 kHz class is the identity geometry; a ninth class, a second
//     16 kHz class, two classes of one rate and every refusal of a class on its own (11025 Hz, 16000 -> 16000 ...) are refused with
//     the class named; a class id out of range is refused with its index named;
//   * the ragged layout for random class assignments: offsets are the running sum of the streams' own frame lengths, the total is
//     the last offset and never above rates_layout_max;
//   * the staged size: the maximum over the resampling classes of hist + F + WW_RATE_PAD, nothing for the 16 kHz class, refused
//     above WW_RATE_STAGE_MAX;
//   * over random tick / freeze / move / reset scripts: a stream's control words are rate_advance's of ITS OWN class at its own
//     count, a move or a reset zeroes the count, a fed packet advances by rate_advance's count (the 16 kHz class: by the packet);
//   * the feed grouping: a partition of the call's packets that keeps each class's packets in the call's order.
// Prints one "geom <rate> <up> <down> <half> <F> <D> <history>" line per class and one "layout <S> <classes...> | <offsets...>" line per
// layout case (for the Python test, which holds them against wwhip.resample.design), then "ok <checks>", and exits 0; or says what
// failed and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "stream_rates.h"

static long n_checks = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    ++n_checks;                                                                  \
    if (!(cond)) {                                                               \
      fprintf(stderr, "stream_rates_check: %s (line %d)\n", #cond, __LINE__);   \
      exit(1);                                                                   \
    }                                                                            \
  } while (0)

// the filter's length as ww_resampler_create and wwhip.resample.design state it (default filter)
static void design(int rate_in, int64_t &up, int64_t &down, int64_t &half, int64_t &tpp) {
  const int zeros = 32;
  const double rolloff = 0.945;
  const int64_t g = std::gcd((int64_t)rate_in, (int64_t)16000);
  up = 16000 / g;
  down = rate_in / g;
  const double L = (double)((int64_t)rate_in * up), f2 = rolloff * (double)(rate_in < 16000 ? rate_in : 16000) / L;
  half = (int64_t)std::ceil((double)zeros / f2);
  tpp = (2 * half + 1 + up - 1) / up;
}

static unsigned long long rng_state = 0x2545f4914f6cdd1dull;
static unsigned rnd(unsigned n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)((rng_state >> 33) % n);
}

static int add(rates_table &t, int rate, char *why, size_t cap) {  // rate 16000: the NULL class
  if (rate == 16000) return rates_add_class(t, true, 0, 0, 0, 0, 0, 0, why, cap);
  int64_t up, down, half, tpp;
  design(rate, up, down, half, tpp);
  return rates_add_class(t, false, rate, 16000, up, down, half, tpp, why, cap);
}

int main() {
  char why[320] = {0};
  const int rates[] = {48000, 16000, 44100, 8000, 22050, 32000, 96000, 192000};
  rates_table t;
  for (int k = 0; k < 8; ++k) {
    CHECK(add(t, rates[k], why, sizeof why) == 0 && t.K == k + 1);
    const rate_geom &g = t.g[k];
    printf("geom %d %lld %lld %lld %d %d %d\n", g.rate_in, (long long)g.up, (long long)g.down, (long long)g.half, g.F, g.D, g.hist);
    CHECK(g.rate_in == rates[k] && g.F * 50 == rates[k]);
    if (rates[k] == 16000) {
      CHECK(t.pass[k] && g.up == 1 && g.down == 1 && g.half == 0 && g.tpp == 0 && g.D == 0 && g.hist == 0 && g.F == 320);
    } else {
      int64_t up, down, half, tpp;
      design(rates[k], up, down, half, tpp);
      rate_geom want;
      CHECK(rate_make_geom(rates[k], 16000, up, down, half, tpp, want, why, sizeof why) == 0);
      CHECK(!t.pass[k] && g.up == want.up && g.down == want.down && g.half == want.half && g.tpp == want.tpp && g.F == want.F && g.D == want.D &&
            g.hist == want.hist);
    }
  }
  // ---- refusals among the classes and of a class on its own, each with the class named
  CHECK(add(t, 24000, why, sizeof why) == 1 && strstr(why, "class 8") && strstr(why, "at most 8"));
  {
    rates_table u;
    CHECK(add(u, 48000, why, sizeof why) == 0 && add(u, 16000, why, sizeof why) == 0);
    CHECK(add(u, 48000, why, sizeof why) == 1 && strstr(why, "class 2") && strstr(why, "same input rate") && strstr(why, "48000"));
    CHECK(add(u, 16000, why, sizeof why) == 1 && strstr(why, "class 2") && strstr(why, "NULL class"));
    CHECK(add(u, 11025, why, sizeof why) == 1 && strstr(why, "class 2") && strstr(why, "fractional") && strstr(why, "220.5"));
    CHECK(rates_add_class(u, false, 16000, 16000, 1, 1, 0, 0, why, sizeof why) == 1 && strstr(why, "class 2") && strstr(why, "plain bank"));
    CHECK(rates_add_class(u, false, 48000, 8000, 1, 6, 204, 409, why, sizeof why) == 1 && strstr(why, "output rate"));
    CHECK(rates_add_class(u, false, 384000, 16000, 1, 24, 24 * 600, 24 * 1200 + 1, why, sizeof why) == 1 && strstr(why, "staged"));
    CHECK(u.K == 2);  // a refused class leaves the table as it was
    const int32_t ids[5] = {0, 1, 1, 2, 0}, neg[2] = {0, -1};
    CHECK(rates_check_ids(u, ids, 3, "stream_rate", why, sizeof why) == 0 && rates_check_ids(u, nullptr, 5, "stream_rate", why, sizeof why) == 0);
    CHECK(rates_check_ids(u, ids, 5, "stream_rate", why, sizeof why) == 1 && strstr(why, "stream_rate[3] = 2") && strstr(why, "0..1"));
    CHECK(rates_check_ids(u, neg, 2, "stream_rate", why, sizeof why) == 1 && strstr(why, "stream_rate[1] = -1"));
  }

  // ---- the staged size
  {
    int64_t stage = -1, want = 0;
    CHECK(rates_stage(t, &stage, why, sizeof why) == 0);
    for (int k = 0; k < t.K; ++k)
      if (!t.pass[k]) want = std::max<int64_t>(want, (int64_t)t.g[k].hist + t.g[k].F + WW_RATE_PAD);
    CHECK(stage == want && stage == (int64_t)t.g[7].hist + 3840 + WW_RATE_PAD && stage * 4 < 19200);  // 192 kHz: 18.7 KB
    rates_table only16;
    CHECK(add(only16, 16000, why, sizeof why) == 0 && rates_stage(only16, &stage, why, sizeof why) == 0 && stage == 0);
    rates_table big = t;
    big.g[2].hist = WW_RATE_STAGE_MAX - big.g[2].F - WW_RATE_PAD;
    CHECK(rates_stage(big, &stage, why, sizeof why) == 0 && stage == WW_RATE_STAGE_MAX);
    big.g[2].hist += 1;
    CHECK(rates_stage(big, &stage, why, sizeof why) == 1 && strstr(why, "class 2") && strstr(why, "staged"));
  }

  // ---- the ragged layout: the issue's mix first, then random assignments
  for (int trial = 0; trial < 200; ++trial) {
    const int fixed[7] = {0, 1, 2, 3, 4, 1, 0};  // 48000, 16000, 44100, 8000, 22050, 16000, 48000
    const int S = trial == 0 ? 7 : 1 + (int)rnd(40);
    std::vector<int32_t> cls((size_t)S), fs((size_t)S);
    std::vector<int64_t> fo((size_t)S + 1);
    for (int s = 0; s < S; ++s) cls[(size_t)s] = trial == 0 ? fixed[s] : (int32_t)rnd((unsigned)t.K);
    const int64_t total = rates_layout(t, cls.data(), S, fs.data(), fo.data());
    int64_t at = 0;
    for (int s = 0; s < S; ++s) {
      CHECK(fs[(size_t)s] == rates[cls[(size_t)s]] / 50 && fo[(size_t)s] == at);
      at += fs[(size_t)s];
    }
    CHECK(fo[(size_t)S] == at && total == at && total <= rates_layout_max(t, S) && rates_layout_max(t, S) == (int64_t)S * 3840);
    CHECK(rates_layout(t, cls.data(), S, nullptr, nullptr) == total);
    if (trial < 4) {
      printf("layout %d", S);
      for (int s = 0; s < S; ++s) printf(" %d", rates[cls[(size_t)s]]);
      printf(" |");
      for (int s = 0; s <= S; ++s) printf(" %lld", (long long)fo[(size_t)s]);
      printf("\n");
    }
    if (trial == 0) {  // byte offsets 0, 1920, 2560, 4324, 4644, 5526, 6166: modulo 16 they are 0, 0, 0, 4, 4, 6, 6
      const int64_t want[8] = {0, 960, 1280, 2162, 2322, 2763, 3083, 4043};
      for (int s = 0; s <= 7; ++s) CHECK(fo[(size_t)s] == want[s]);
    }
  }

  // ---- a stream's control words and counts over random scripts of ticks, frozen ticks, packets, moves and resets: always those of
  //      the single-rate bank of the stream's class at the stream's own count
  for (int trial = 0; trial < 300; ++trial) {
    int32_t c = (int32_t)rnd((unsigned)t.K);
    int64_t n = 0;
    for (int step = 0; step < 120; ++step) {
      const unsigned kind = rnd(16);
      if (kind == 0) {  // a move
        const int32_t to = (int32_t)rnd((unsigned)t.K);
        n += 1;  // (whatever the count was)
        rates_move(c, n, to);
        CHECK(c == to && n == 0);
      } else if (kind == 1) {  // a reset: a move to the stream's own class
        rates_move(c, n, c);
        CHECK(n == 0);
      } else if (kind == 2) {  // a frozen tick: nothing is asked, nothing moves
      } else if (kind < 6) {   // a fed packet
        const int64_t k = kind == 3 ? 0 : kind == 4 ? 1 : 1 + rnd(3000);
        const int64_t adv = rates_advance(t, c, n, k);
        if (t.pass[c]) {
          CHECK(adv == k);
        } else {
          CHECK(adv == rate_advance(t.g[c], n, k).count);
          n += k;
        }
      } else {  // a tick
        const int64_t before = n;
        const rate_ctl rc = rates_tick(t, c, n);
        if (t.pass[c]) {
          CHECK(rc.res == 0 && rc.zeros == 0 && rc.held == 0 && rc.pad == 0 && n == 0 && before == 0);
        } else {
          const rate_step st = rate_advance(t.g[c], before, t.g[c].F);
          CHECK(st.count == 320 && rc.res == st.res && rc.zeros == st.zeros && rc.held == st.held && rc.pad == 0 && n == before + t.g[c].F);
          if (before == 0) CHECK(rc.held == 0 && rc.res == 0 && rc.zeros == t.g[c].D);
        }
        CHECK(rates_advance(t, c, before, t.g[c].F) == 320);
      }
    }
  }

  // ---- the feed grouping
  for (int trial = 0; trial < 300; ++trial) {
    const int n = (int)rnd(50), K = 1 + (int)rnd(8);
    std::vector<int32_t> pc((size_t)n);
    for (int i = 0; i < n; ++i) pc[(size_t)i] = (int32_t)rnd((unsigned)K);
    rates_groups g;
    g.order.assign(3, 77);  // (what an earlier call left)
    rates_group(pc.data(), n, g);
    CHECK((int)g.order.size() == n && g.start[0] == 0 && g.start[WW_STREAM_MAX_RATES] == n);
    std::vector<int> seen((size_t)n, 0);
    for (int c = 0; c < WW_STREAM_MAX_RATES; ++c) {
      CHECK(g.start[c] <= g.start[c + 1]);
      for (int j = g.start[c]; j < g.start[c + 1]; ++j) {
        const int i = g.order[(size_t)j];
        CHECK(i >= 0 && i < n && pc[(size_t)i] == c && ++seen[(size_t)i] == 1);
        if (j > g.start[c]) CHECK(g.order[(size_t)j - 1] < i);  // the call's order within the class
      }
    }
    for (int i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1);
  }
  printf("ok %ld\n", n_checks);
  return 0;
}
