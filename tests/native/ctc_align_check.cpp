// ctc_align_check.cpp - csrc/ctc_align.h's Viterbi alignment as a host program (tests/test_ctc_align_native.py builds it with
// Address + UB sanitizer and runs it as a child process).  Input file: int32 n, then per table int32 T, L, U, the U int32 labels of
// the target and T * L float32 posteriors (row-major).  Every table lies in a heap block of exactly its size, the target in one of
// exactly U words and the span in one of exactly 18 bytes, so an access past any end is a sanitizer report.  Per table and mode:
//   - the span is also written between guard bytes, which must survive, from a buffer whose 18 bytes were all different from -1
//     before the call (all 18 are written);
//   - the same table laid out with ld = L + 3 (the gaps poisoned with NaN) must give the same bits;
//   - where L^T <= 4096 (T <= 6 at L <= 4), every path is enumerated in double: the value lies within (T - 1) 2^-24 of the best
//     admissible path's probability, and where the best leads the second by more than 1e-5 relative the spans are that path's.
// Output: one line per table, "<exact value bits> <prefix value bits> <18 exact span bytes> <18 prefix span bytes>" (the spans as
// signed decimals), and a last line "ok <n> enumerated <m>".  Exit 3 on a mismatch, 2 on a refused table.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ctc_align.h"

static bool rd(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

static unsigned bits(float v) {
  unsigned u;
  memcpy(&u, &v, 4);
  return u;
}

// the collapse of path[0 .. n): repeats merged, blanks dropped; returns its length (at most n)
static int collapse(const int *path, int n, int blank, int *out) {
  int m = 0, prev = -1;
  for (int t = 0; t < n; ++t) {
    if (path[t] != blank && path[t] != prev) out[m++] = path[t];
    prev = path[t];
  }
  return m;
}

struct best_path {
  double p = 0.0, second = 0.0;
  int len = 0, path[8];
};

// Every admissible path in double.  Exact: the paths of T steps whose collapse is c.  Prefix: the paths of 1 .. T steps whose collapse
// is c and whose last step completes it.  The most probable, the shortest among equals.
static best_path enumerate(const float *y, int T, int L, const int32_t *c, int U, int mode) {
  best_path b;
  for (int n = (mode == WW_CTC_SCORE_EXACT ? T : 1); n <= T; ++n) {
    long long total = 1;
    for (int t = 0; t < n; ++t) total *= L;
    for (long long code = 0; code < total; ++code) {
      int path[8], out[8];
      long long r = code;
      for (int t = 0; t < n; ++t) path[t] = (int)(r % L), r /= L;
      int m = collapse(path, n, L - 1, out);
      bool ok = m == U;
      for (int u = 0; ok && u < U; ++u) ok = out[u] == c[u];
      if (ok && mode == WW_CTC_SCORE_PREFIX && n > 1) {
        m = collapse(path, n - 1, L - 1, out);
        bool before = m == U;
        for (int u = 0; before && u < U; ++u) before = out[u] == c[u];
        ok = !before;
      }
      if (!ok) continue;
      double p = 1.0;
      for (int t = 0; t < n; ++t) p *= (double)y[t * L + path[t]];
      if (p > b.p) {
        b.second = b.p;
        b.p = p;
        b.len = n;
        memcpy(b.path, path, sizeof path);
      } else if (p > b.second) {
        b.second = p;
      }
    }
  }
  return b;
}

static int fail(int i, int mode, const char *what) {
  fprintf(stderr, "table %d mode %d: %s\n", i, mode, what);
  return 3;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: ctc_align_check <tables.bin>\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  int32_t n = 0;
  if (!rd(f, &n, 4) || n < 0) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  int enumerated = 0;
  for (int32_t i = 0; i < n; ++i) {
    int32_t h[3];
    if (!rd(f, h, sizeof h) || h[2] < 1 || h[2] > WW_CTC_SCORE_MAX_TARGET) {
      fprintf(stderr, "table %d: bad header\n", (int)i);
      return 2;
    }
    const int T = h[0], L = h[1], U = h[2];
    int32_t *c = (int32_t *)malloc((size_t)U * sizeof(int32_t));
    if (!c || !rd(f, c, (size_t)U * sizeof(int32_t))) {
      fprintf(stderr, "table %d: short read\n", (int)i);
      return 2;
    }
    int32_t padded[WW_CTC_SCORE_MAX_TARGET] = {0};
    memcpy(padded, c, (size_t)U * sizeof(int32_t));
    char why[200];
    if (!ww_ctc_score_args_ok(T, L, padded, &h[2], 1, WW_CTC_SCORE_PREFIX, why, sizeof why)) {
      fprintf(stderr, "table %d: %s\n", (int)i, why);
      free(c);
      fclose(f);
      return 2;
    }
    float *steps = (float *)malloc((size_t)T * L * sizeof(float));
    if (!steps || !rd(f, steps, (size_t)T * L * sizeof(float))) {
      fprintf(stderr, "table %d: short read\n", (int)i);
      return 2;
    }
    const int ld = L + 3;
    float *wide = (float *)malloc(((size_t)(T - 1) * ld + L) * sizeof(float));  // (the last row has no gap behind it)
    for (int t = 0; t < T; ++t) {
      memcpy(wide + (size_t)t * ld, steps + (size_t)t * L, (size_t)L * sizeof(float));
      if (t + 1 < T)
        for (int j = L; j < ld; ++j) wide[(size_t)t * ld + j] = NAN;
    }
    float value[2];
    int8_t *span[2];
    for (int mode = 0; mode < 2; ++mode) {
      span[mode] = (int8_t *)malloc(18);
      memset(span[mode], 0x55, 18);
      ww_ctc_align_row(steps, T, L, L, c, U, mode, &value[mode], span[mode]);
      int8_t guarded[4 + 18 + 4];
      memset(guarded, 0x55, sizeof guarded);
      float v2 = -1.0f;
      ww_ctc_align_row(wide, T, L, ld, c, U, mode, &v2, guarded + 4);
      for (int j = 0; j < 4; ++j)
        if (guarded[j] != 0x55 || guarded[22 + j] != 0x55) return fail(i, mode, "a guard byte around the span was written");
      if (bits(v2) != bits(value[mode]) || memcmp(guarded + 4, span[mode], 18)) return fail(i, mode, "ld = L + 3 gives other bits than ld = L");
      for (int j = 0; j < 18; ++j)
        if (span[mode][j] == 0x55) return fail(i, mode, "a span byte was not written");
      for (int u = U; u < WW_CTC_SCORE_MAX_TARGET; ++u)
        if (span[mode][2 * u] != -1 || span[mode][2 * u + 1] != -1) return fail(i, mode, "a row past U is not -1");
      long long paths = 1;
      for (int t = 0; t < T && paths <= 4096; ++t) paths *= L;
      if (T <= 6 && paths <= 4096) {
        const best_path b = enumerate(steps, T, L, c, U, mode);
        ++enumerated;
        if (std::fabs((double)value[mode] - b.p) > (T - 1) * std::ldexp(1.0, -24) * b.p + 1e-37) return fail(i, mode, "the value is not the best path's probability");
        if (b.p == 0.0) {
          for (int j = 0; j < 18; ++j)
            if (span[mode][j] != -1) return fail(i, mode, "no path, but a span");
        } else if (b.p - b.second > 1e-5 * b.p) {
          int8_t want[18];
          memset(want, -1, 18);
          int u = -1, prev = -1;
          for (int t = 0; t < b.len; ++t) {
            const int k = b.path[t];
            if (k != L - 1 && k != prev) ++u, want[2 * u] = (int8_t)t;
            if (k != L - 1) want[2 * u + 1] = (int8_t)t;
            prev = k;
          }
          if (memcmp(want, span[mode], 18)) return fail(i, mode, "the spans are not the best path's");
        }
      }
    }
    printf("%08x %08x", bits(value[0]), bits(value[1]));
    for (int mode = 0; mode < 2; ++mode)
      for (int j = 0; j < 18; ++j) printf(" %d", (int)span[mode][j]);
    printf("\n");
    free(span[0]);
    free(span[1]);
    free(wide);
    free(steps);
    free(c);
  }
  fclose(f);
  printf("ok %d enumerated %d\n", (int)n, enumerated);
  return 0;
}
