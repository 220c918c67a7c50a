// stream_formats_check - csrc/stream_formats.h (the host-only bookkeeping of a stream bank whose rate classes read int16 or G.711
// samples) alone on the CPU, under Address + UB sanitizer (tests/test_g711_host.py compiles and runs it; nothing here touches a GPU):
//   * the class table: a class is a (rate, format) pair - one rate in two formats passes, the same pair twice, a float32 class, an
//     unknown format, a ninth class and every refusal of a class on its own are refused with the class named and the table left alone;
//   * the byte layout for random class assignments: an int16 frame starts on an even byte, a G.711 frame on ANY byte (odd ones are
//     met), a gap between two frames is one pad byte and lies in front of an int16 frame only, offsets ascend, the total is the end of
//     the last frame = the frames' bytes + the pad bytes;
//   * the reserved size: formats_layout_max bounds the layout after every step of random move scripts;
//   * a bank of int16 classes only: the layout is 2 x stream_rates.h's sample layout, its maximum 2 x rates_layout_max, and it has no
//     pad byte (the sample offsets of such a bank are its byte offsets halved);
//   * the packet checks: an int16 packet with an odd offset or an odd length is refused with the packet named, a G.711 packet starts
//     and ends anywhere, the sample counts are bytes / bytes per sample.
// Prints "layout <S> <frame bytes...> | <byte offsets...>" for the mix of tests/test_gpu_g711_streams.py, then "ok <checks>", and exits 0;
// or says what failed and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "stream_formats.h"

static long n_checks = 0;
#define CHECK(cond)                                                               \
  do {                                                                            \
    ++n_checks;                                                                   \
    if (!(cond)) {                                                                \
      fprintf(stderr, "stream_formats_check: %s (line %d)\n", #cond, __LINE__);  \
      exit(1);                                                                    \
    }                                                                             \
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

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)((rng_state >> 33) % n);
}

static int add(rates_table &t, formats_table &f, int rate, int fmt, char *why, size_t cap) {  // rate 16000: the NULL class of the format
  if (rate == 16000) return formats_add_class(t, f, fmt, true, 0, 0, 0, 0, 0, 0, why, cap);
  int64_t up, down, half, tpp;
  design(rate, up, down, half, tpp);
  return formats_add_class(t, f, fmt, false, rate, 16000, up, down, half, tpp, why, cap);
}

// every property of one layout
static void check_layout(const rates_table &t, const formats_table &f, const std::vector<int32_t> &cls, bool *odd_g711, bool *padded) {
  const int S = (int)cls.size();
  std::vector<int32_t> fb((size_t)S), fm((size_t)S);
  std::vector<int64_t> bo((size_t)S + 1);
  const int64_t total = formats_layout(t, f, cls.data(), S, fb.data(), bo.data(), fm.data());
  CHECK(total == bo[(size_t)S] && total == formats_layout(t, f, cls.data(), S, nullptr, nullptr, nullptr));
  CHECK(total <= formats_layout_max(t, f, S));
  int64_t end = 0, sum = 0, pads = 0;
  for (int s = 0; s < S; ++s) {
    const int c = cls[(size_t)s], b = format_bytes(f.fmt[c]);
    CHECK(fm[(size_t)s] == f.fmt[c] && fb[(size_t)s] == t.g[c].F * b && (b == 1 || b == 2));
    const int64_t gap = bo[(size_t)s] - end;
    CHECK(gap == 0 || gap == 1);          // offsets ascend: a frame starts at the end of the one before, or one byte behind it
    if (b == 2) CHECK(bo[(size_t)s] % 2 == 0 && gap == (end & 1));
    else CHECK(gap == 0);                 // no pad byte in front of a G.711 frame
    if (b == 1 && (bo[(size_t)s] & 1)) *odd_g711 = true;
    pads += gap;
    sum += fb[(size_t)s];
    end = bo[(size_t)s] + fb[(size_t)s];
  }
  CHECK(end == total && total == sum + pads);
  if (pads) *padded = true;
}

int main() {
  char why[320] = {0};
  // ---- the class table: the mix of the GPU test (8050 Hz: up 320, down 161 - a frame of 161 samples)
  const int rate[7] = {8000, 8000, 8000, 16000, 16000, 8050, 48000};
  const int fmt[7] = {WW_FMT_MULAW, WW_FMT_ALAW, WW_FMT_I16, WW_FMT_MULAW, WW_FMT_I16, WW_FMT_MULAW, WW_FMT_I16};
  rates_table t;
  formats_table f;
  CHECK(!f.g711);
  for (int k = 0; k < 7; ++k) {
    CHECK(add(t, f, rate[k], fmt[k], why, sizeof why) == 0 && t.K == k + 1 && f.fmt[k] == fmt[k]);
    CHECK(t.g[k].rate_in == rate[k] && t.g[k].F * 50 == rate[k] && t.pass[k] == (rate[k] == 16000));
  }
  CHECK(f.g711 && t.g[5].up == 320 && t.g[5].down == 161 && t.g[5].F == 161);
  CHECK(format_bytes(WW_FMT_I16) == 2 && format_bytes(WW_FMT_MULAW) == 1 && format_bytes(WW_FMT_ALAW) == 1 && format_bytes(1) == 0 && format_bytes(2) == 0 &&
        format_bytes(10) == 0);
  CHECK(add(t, f, 8000, WW_FMT_ALAW, why, sizeof why) == 1 && strstr(why, "class 7") && strstr(why, "same input rate and format") && strstr(why, "class 1"));
  CHECK(add(t, f, 16000, WW_FMT_MULAW, why, sizeof why) == 1 && strstr(why, "class 7") && strstr(why, "class 3"));
  CHECK(add(t, f, 16000, WW_FMT_I16, why, sizeof why) == 1 && strstr(why, "class 4"));
  CHECK(add(t, f, 44100, 1, why, sizeof why) == 1 && strstr(why, "class 7") && strstr(why, "format 1") && strstr(why, "float32"));
  CHECK(add(t, f, 44100, 2, why, sizeof why) == 1 && strstr(why, "format 2"));
  CHECK(add(t, f, 11025, WW_FMT_MULAW, why, sizeof why) == 1 && strstr(why, "class 7") && strstr(why, "fractional"));
  CHECK(formats_add_class(t, f, WW_FMT_ALAW, false, 16000, 16000, 1, 1, 0, 0, why, sizeof why) == 1 && strstr(why, "plain bank"));
  CHECK(t.K == 7);  // a refused class leaves the table as it was
  CHECK(add(t, f, 16000, WW_FMT_ALAW, why, sizeof why) == 0 && t.K == 8);  // a third 16 kHz class, in a third format
  CHECK(add(t, f, 32000, WW_FMT_I16, why, sizeof why) == 1 && strstr(why, "class 8") && strstr(why, "at most 8"));

  // ---- the layout of the GPU test's bank, stream s in class s
  {
    std::vector<int32_t> cls = {0, 1, 2, 3, 4, 5, 6};
    int32_t fb[7];
    int64_t bo[8];
    CHECK(formats_layout(t, f, cls.data(), 7, fb, bo, nullptr) == bo[7]);
    printf("layout 7");
    for (int s = 0; s < 7; ++s) printf(" %d", fb[s]);
    printf(" |");
    for (int s = 0; s <= 7; ++s) printf(" %lld", (long long)bo[s]);
    printf("\n");
    // 160 + 160 + 320 + 320 + 640 + 161 | pad | 1920
    CHECK(bo[5] == 1600 && bo[6] == 1762 && bo[7] == 1762 + 1920);
    bool odd = false, padded = false;
    check_layout(t, f, cls, &odd, &padded);
    CHECK(padded);
  }

  // ---- random assignments and move scripts: every layout has the properties, and the reserved size bounds each
  bool odd = false, padded = false;
  for (int it = 0; it < 300; ++it) {
    const int S = 1 + (int)rnd(40);
    std::vector<int32_t> cls((size_t)S);
    for (int s = 0; s < S; ++s) cls[(size_t)s] = (int32_t)rnd((unsigned)t.K);
    check_layout(t, f, cls, &odd, &padded);
    for (int step = 0; step < 30; ++step) {
      const int count = 1 + (int)rnd(4), c = (int)rnd((unsigned)t.K);
      for (int j = 0; j < count; ++j) {
        int64_t n = 7;
        rates_move(cls[(size_t)rnd((unsigned)S)], n, c);
        CHECK(n == 0);
      }
      check_layout(t, f, cls, &odd, &padded);
    }
    // the worst case is met: every stream an odd G.711 frame, then int16 ones alternate
    std::fill(cls.begin(), cls.end(), 6);
    CHECK(formats_layout(t, f, cls.data(), S, nullptr, nullptr, nullptr) == (int64_t)S * 1920 && (int64_t)S * 1920 < formats_layout_max(t, f, S));
  }
  CHECK(odd && padded);

  // ---- int16 classes only: twice stream_rates.h's layout
  {
    const int r16[4] = {48000, 16000, 8000, 44100};
    rates_table a, b;
    formats_table g;
    for (int k = 0; k < 4; ++k) {
      CHECK(add(a, g, r16[k], WW_FMT_I16, why, sizeof why) == 0);
      int64_t up, down, half, tpp;
      design(r16[k], up, down, half, tpp);
      CHECK((r16[k] == 16000 ? rates_add_class(b, true, 0, 0, 0, 0, 0, 0, why, sizeof why)
                             : rates_add_class(b, false, r16[k], 16000, up, down, half, tpp, why, sizeof why)) == 0);
    }
    CHECK(!g.g711);
    CHECK(add(a, g, 8000, WW_FMT_I16, why, sizeof why) == 1 && strstr(why, "same input rate"));
    for (int it = 0; it < 100; ++it) {
      const int S = 1 + (int)rnd(30);
      std::vector<int32_t> cls((size_t)S), fs((size_t)S), fb((size_t)S), fm((size_t)S);
      std::vector<int64_t> so((size_t)S + 1), bo((size_t)S + 1);
      for (int s = 0; s < S; ++s) cls[(size_t)s] = (int32_t)rnd(4);
      const int64_t ns = rates_layout(b, cls.data(), S, fs.data(), so.data()), nb = formats_layout(a, g, cls.data(), S, fb.data(), bo.data(), fm.data());
      CHECK(nb == 2 * ns && formats_layout_max(a, g, S) == 2 * rates_layout_max(b, S));
      for (int s = 0; s <= S; ++s) CHECK(bo[(size_t)s] == 2 * so[(size_t)s]);
      for (int s = 0; s < S; ++s) CHECK(fb[(size_t)s] == 2 * fs[(size_t)s] && fm[(size_t)s] == WW_FMT_I16);
      // no pad byte anywhere in a table without G.711: a frame starts where the one before ends, so the sample offsets are bo / 2
      bool odd16 = false, padded16 = false;
      check_layout(a, g, cls, &odd16, &padded16);
      CHECK(!padded16 && !odd16);
      for (int s = 0; s < S; ++s) CHECK(bo[(size_t)s + 1] == bo[(size_t)s] + fb[(size_t)s]);
    }
  }

  // ---- the packet checks
  {
    int64_t k = -1;
    CHECK(formats_packet(WW_FMT_I16, 3, 10, 10, &k, why, sizeof why) == 0 && k == 0);
    CHECK(formats_packet(WW_FMT_I16, 3, 10, 650, &k, why, sizeof why) == 0 && k == 320);
    CHECK(formats_packet(WW_FMT_I16, 3, 11, 651, &k, why, sizeof why) == 1 && strstr(why, "packet 3") && strstr(why, "odd offset") && strstr(why, "11"));
    CHECK(formats_packet(WW_FMT_I16, 4, 10, 13, &k, why, sizeof why) == 1 && strstr(why, "packet 4") && strstr(why, "odd length") && strstr(why, "3 bytes"));
    CHECK(k == 320);  // a refusal writes no count
    for (int it = 0; it < 2000; ++it) {
      const int64_t b0 = rnd(100000), n = rnd(5000);
      const int fm = rnd(2) ? WW_FMT_MULAW : WW_FMT_ALAW;
      CHECK(formats_packet(fm, it, b0, b0 + n, &k, why, sizeof why) == 0 && k == n);
      const int r = formats_packet(WW_FMT_I16, it, b0, b0 + n, &k, why, sizeof why);
      CHECK(r == (((b0 | n) & 1) ? 1 : 0));
      if (!r) CHECK(k * 2 == n);
    }
    CHECK(formats_packet(WW_FMT_MULAW, 0, 9, 5, &k, why, sizeof why) == 0 && k == -4);  // descending offsets: a negative count, the caller's refusal
  }
  printf("ok %ld\n", n_checks);
  return 0;
}
