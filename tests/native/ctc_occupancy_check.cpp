// ctc_occupancy_check.cpp - csrc/ctc_occupancy.h's forward-backward occupancy as a host program (tests/test_ctc_occupancy_native.py
// builds it with Address + UB sanitizer and runs it as a child process).  Input file: int32 n, then per table int32 T, L, U, the U
// int32 labels of the target and T * L float32 posteriors (row-major).  Every table lies in a heap block of exactly its size, the
// target in one of exactly U words, occ in one of exactly T * 9 floats and cls in one of exactly T * L, so an access past any end is
// a sanitizer report.  Per table and mode:
//   - occ and cls are also written between guard words, which must survive, from the same table laid out with ld = L + 3 (the gaps
//     poisoned with NaN), and must carry the same bits as with ld = L; every word of both was a canary before the call and is not
//     after it; rows u >= U of occ are +0; Z == 0 leaves +0 everywhere;
//   - where L^T <= 4096 (T <= 6 at L <= 4), every path is enumerated in double: Z, every occ and every cls entry lie within the
//     bound of tests/ctc_occupancy64.py of the enumeration's.
// Output: one line per table of 8-digit hex words - Z exact, Z prefix, occ exact [T][9], cls exact [T][L], occ prefix [T][9] - and a
// last line "ok <n> enumerated <m>".  Exit 3 on a mismatch, 2 on a refused table.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ctc_occupancy.h"

static const unsigned CANARY = 0x55555555u;  // (1.5e13 as a float: no occupancy)
static const int NU = WW_CTC_SCORE_MAX_TARGET;

static bool rd(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

static unsigned bits(float v) {
  unsigned u;
  memcpy(&u, &v, 4);
  return u;
}

static float *canaried(size_t words) {
  float *p = (float *)malloc(words * sizeof(float));
  for (size_t j = 0; p && j < words; ++j) memcpy(p + j, &CANARY, 4);
  return p;
}

static int fail(int i, int mode, const char *what) {
  fprintf(stderr, "table %d mode %d: %s\n", i, mode, what);
  return 3;
}

// Every path of T steps in double: Z, occ [T][9] and cls [T][L] (not yet divided by Z).  Exact: the paths whose collapse is c.  Prefix:
// the paths whose collapse starts with c, each completing prefix counted once (the steps behind it all class 0) with the product up
// to its completing step, which counts for column U - 1 alone.
static void enumerate(const float *y, int T, int L, const int32_t *c, int U, int mode, double *Z, double *occ, double *cls) {
  *Z = 0.0;
  for (int j = 0; j < T * NU; ++j) occ[j] = 0.0;
  for (int j = 0; j < T * L; ++j) cls[j] = 0.0;
  long long total = 1;
  for (int t = 0; t < T; ++t) total *= L;
  for (long long code = 0; code < total; ++code) {
    int path[8], where[8], m = 0, prev = -1, done = -1;
    long long r = code;
    bool ok = true;
    for (int t = 0; t < T; ++t) path[t] = (int)(r % L), r /= L;
    for (int t = 0; t < T; ++t) {
      if (path[t] != L - 1 && path[t] != prev) {
        if (m < U && path[t] != c[m]) ok = false;
        if (++m == U && ok && done < 0) done = t;
      }
      where[t] = path[t] != L - 1 ? m - 1 : -1;
      prev = path[t];
    }
    if (!ok || done < 0) continue;
    int last = T - 1;
    if (mode == WW_CTC_SCORE_PREFIX) {
      bool zeros = true;
      for (int t = done + 1; t < T; ++t) zeros = zeros && path[t] == 0;
      if (!zeros) continue;
      last = done;
    } else if (m != U) {
      continue;
    }
    double p = 1.0;
    for (int t = 0; t <= last; ++t) p *= (double)y[t * L + path[t]];
    *Z += p;
    for (int t = 0; t <= last; ++t) {
      if (mode == WW_CTC_SCORE_EXACT) cls[t * L + path[t]] += p;
      if (mode == WW_CTC_SCORE_PREFIX && t == done) occ[t * NU + U - 1] += p;
      else if (where[t] >= 0) occ[t * NU + where[t]] += p;
    }
  }
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: ctc_occupancy_check <tables.bin>\n");
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
    float dummy = 0.0f;
    if (!ww_ctc_occupancy_args_ok(T, L, padded, &h[2], 1, WW_CTC_SCORE_PREFIX, &dummy, &dummy, nullptr, why, sizeof why)) {
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
    const size_t n_occ = (size_t)T * NU, n_cls = (size_t)T * L;
    float Z[2], *occ[2], *cls = nullptr;
    for (int mode = 0; mode < 2; ++mode) {
      const bool with_cls = mode == WW_CTC_SCORE_EXACT;
      occ[mode] = canaried(n_occ);
      if (with_cls) cls = canaried(n_cls);
      Z[mode] = ww_ctc_occupancy_row(steps, T, L, L, c, U, mode, occ[mode], with_cls ? cls : nullptr);
      float *g_occ = canaried(n_occ + 8), *g_cls = canaried(n_cls + 8);
      const float Z2 = ww_ctc_occupancy_row(wide, T, L, ld, c, U, mode, g_occ + 4, with_cls ? g_cls + 4 : nullptr);
      for (int j = 0; j < 4; ++j) {
        if (bits(g_occ[j]) != CANARY || bits(g_occ[4 + n_occ + j]) != CANARY) return fail(i, mode, "a guard word around occ was written");
        if (bits(g_cls[j]) != CANARY || bits(g_cls[4 + n_cls + j]) != CANARY) return fail(i, mode, "a guard word around cls was written");
      }
      if (!with_cls)
        for (size_t j = 0; j < n_cls; ++j)
          if (bits(g_cls[4 + j]) != CANARY) return fail(i, mode, "cls was written though none was passed");
      if (bits(Z2) != bits(Z[mode]) || memcmp(g_occ + 4, occ[mode], n_occ * 4) || (with_cls && memcmp(g_cls + 4, cls, n_cls * 4)))
        return fail(i, mode, "ld = L + 3 gives other bits than ld = L");
      free(g_occ);
      free(g_cls);
      if (bits(Z[mode]) != bits(ww_ctc_score_row(steps, T, L, L, c, U, mode))) return fail(i, mode, "Z does not carry the score's bits");
      for (size_t j = 0; j < n_occ; ++j) {
        if (bits(occ[mode][j]) == CANARY) return fail(i, mode, "an occ word was not written");
        if ((int)(j % NU) >= U && bits(occ[mode][j]) != 0) return fail(i, mode, "a row past U is not +0");
        if (Z[mode] == 0.0f && bits(occ[mode][j]) != 0) return fail(i, mode, "Z == 0, but an occ entry is not +0");
      }
      for (size_t j = 0; with_cls && j < n_cls; ++j) {
        if (bits(cls[j]) == CANARY) return fail(i, mode, "a cls word was not written");
        if (Z[mode] == 0.0f && bits(cls[j]) != 0) return fail(i, mode, "Z == 0, but a cls entry is not +0");
      }
      long long paths = 1;
      for (int t = 0; t < T && paths <= 4096; ++t) paths *= L;
      if (T <= 6 && paths <= 4096) {
        double Z64, occ64[6 * NU], cls64[6 * 64];  // (T <= 6, L <= 64)
        enumerate(steps, T, L, c, U, mode, &Z64, occ64, cls64);
        ++enumerated;
        const double u24 = std::ldexp(1.0, -24), tiny = std::ldexp(1.0, -126);
        if (std::fabs((double)Z[mode] - Z64) > (3 * T + 2) * u24 * Z64 + (2 * U + 1) * T * tiny) return fail(i, mode, "Z is not the enumeration's");
        if (Z64 > 0.0) {
          const double absolute = 2.0 * (2 * U + 1) * T * tiny / Z64 + std::ldexp(1.0, -149);
          for (size_t j = 0; j < n_occ; ++j) {
            const double g = occ64[j] / Z64;
            if (std::fabs((double)occ[mode][j] - g) > (6 * T + 4) * u24 * g + absolute) return fail(i, mode, "an occ entry is not the enumeration's");
          }
          for (size_t j = 0; with_cls && j < n_cls; ++j) {
            const double g = cls64[j] / Z64;
            if (std::fabs((double)cls[j] - g) > (6 * T + 4 + 2 * U) * u24 * g + (U + 1) * absolute) return fail(i, mode, "a cls entry is not the enumeration's");
          }
        }
      }
    }
    printf("%08x %08x", bits(Z[0]), bits(Z[1]));
    for (size_t j = 0; j < n_occ; ++j) printf(" %08x", bits(occ[0][j]));
    for (size_t j = 0; j < n_cls; ++j) printf(" %08x", bits(cls[j]));
    for (size_t j = 0; j < n_occ; ++j) printf(" %08x", bits(occ[1][j]));
    printf("\n");
    free(occ[0]);
    free(occ[1]);
    free(cls);
    free(wide);
    free(steps);
    free(c);
  }
  fclose(f);
  printf("ok %d enumerated %d\n", (int)n, enumerated);
  return 0;
}
