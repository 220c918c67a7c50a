// ctc_score_check.cpp - csrc/ctc_score.h's forward-algorithm score as a host program (tests/test_ctc_score_native.py builds it with
// Address + UB sanitizer and runs it as a child process).  Input file: int32 n, then per table int32 T, L, U, the U int32 labels of
// the target and T * L float32 posteriors (row-major, T rows of L).  Every table lies in a heap block of exactly its size and the
// target in one of exactly U words, so a read past either end is a sanitizer report.  The argument check of the entry points
// (ww_ctc_score_args_ok) sees every table first.  Output: one line per table, the bits of the two scores in hexadecimal,
//   "<exact> <prefix>"
// and a last line "ok <n>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ctc_score.h"

static bool rd(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

static unsigned bits(float v) {
  unsigned u;
  memcpy(&u, &v, 4);
  return u;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: ctc_score_check <tables.bin>\n");
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
    printf("%08x %08x\n", bits(ww_ctc_score_row(steps, T, L, L, c, U, WW_CTC_SCORE_EXACT)), bits(ww_ctc_score_row(steps, T, L, L, c, U, WW_CTC_SCORE_PREFIX)));
    free(steps);
    free(c);
  }
  fclose(f);
  printf("ok %d\n", (int)n);
  return 0;
}
