// ctc_decode_check.cpp - csrc/ctc_decode.h's greedy decode as a host program (tests/test_ctc_native.py builds it with Address + UB
// sanitizer and runs it as a child process).  Input file: int32 n, then per table int32 T, L, max_labels and T * L float32
// posteriors (row-major, T rows of L).  Every table lies in a heap block of exactly its size and the labels in one of exactly
// max_labels words, so a read or write past either end is a sanitizer report.  Output: one line per table,
//   "<length> <label 0> ... <label max_labels - 1>"
// and a last line "ok <n>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctc_decode.h"

static bool rd(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: ctc_decode_check <tables.bin>\n");
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
    if (!rd(f, h, sizeof h) || h[0] < 1 || h[0] > 4096 || h[1] < 2 || h[1] > 64 || h[2] < 1 || h[2] > h[0]) {
      fprintf(stderr, "table %d: bad header\n", (int)i);
      return 2;
    }
    const int T = h[0], L = h[1], M = h[2];
    float *steps = (float *)malloc((size_t)T * L * sizeof(float));
    int32_t *labels = (int32_t *)malloc((size_t)M * sizeof(int32_t));
    if (!steps || !labels || !rd(f, steps, (size_t)T * L * sizeof(float))) {
      fprintf(stderr, "table %d: short read\n", (int)i);
      return 2;
    }
    memset(labels, 0x5a, (size_t)M * sizeof(int32_t));
    const int32_t len = ww_ctc_greedy_row(steps, T, L, L, labels, M);
    printf("%d", (int)len);
    for (int k = 0; k < M; ++k) printf(" %d", (int)labels[k]);
    printf("\n");
    free(steps);
    free(labels);
  }
  fclose(f);
  printf("ok %d\n", (int)n);
  return 0;
}
