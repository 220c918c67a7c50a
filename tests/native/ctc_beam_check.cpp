// ctc_beam_check.cpp - csrc/ctc_beam.h's prefix beam search as a host program (tests/test_ctc_beam_native.py builds it with
// Address + UB sanitizer and runs it as a child process).  Input file: int32 n, then per table int32 T, L, W, P, M (beam width, top
// paths, max_labels) and T * L float32 posteriors (row-major, T rows of L).  Every table lies in a heap block of exactly its size, and
// so does each of the three outputs, so a read or write past an end is a sanitizer report.  The argument check of the entry points
// (ww_ctc_beam_args_ok) sees every table first.  Output: one line per table, per reported path
//   "<length> <the probability's bits in hexadecimal> <M labels>"
// and a last line "ok <n>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ctc_beam.h"

static bool rd(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

static unsigned bits(float v) {
  unsigned u;
  memcpy(&u, &v, 4);
  return u;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: ctc_beam_check <tables.bin>\n");
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
    int32_t h[5];
    if (!rd(f, h, sizeof h)) {
      fprintf(stderr, "table %d: bad header\n", (int)i);
      return 2;
    }
    const int T = h[0], L = h[1], W = h[2], P = h[3], M = h[4];
    char why[200];
    if (!ww_ctc_beam_args_ok(T, L, W, P, M, why, sizeof why)) {
      fprintf(stderr, "table %d: %s\n", (int)i, why);
      fclose(f);
      return 2;
    }
    float *steps = (float *)malloc((size_t)T * L * sizeof(float));
    int32_t *labels = (int32_t *)malloc((size_t)P * M * sizeof(int32_t)), *lengths = (int32_t *)malloc((size_t)P * sizeof(int32_t));
    float *prob = (float *)malloc((size_t)P * sizeof(float));
    if (!steps || !labels || !lengths || !prob || !rd(f, steps, (size_t)T * L * sizeof(float))) {
      fprintf(stderr, "table %d: short read\n", (int)i);
      return 2;
    }
    ww_ctc_beam_row(steps, T, L, L, W, P, M, labels, lengths, prob);
    for (int p = 0; p < P; ++p) {
      printf("%s%d %08x", p ? " " : "", (int)lengths[p], bits(prob[p]));
      for (int j = 0; j < M; ++j) printf(" %d", (int)labels[p * M + j]);
    }
    printf("\n");
    free(prob);
    free(lengths);
    free(labels);
    free(steps);
  }
  fclose(f);
  printf("ok %d\n", (int)n);
  return 0;
}
