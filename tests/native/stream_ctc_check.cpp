// csrc/stream_ctc.h on the host, alone: built with -fsanitize=address,undefined and run as a child process by
// tests/test_stream_ctc_host.py.
//   stream_ctc_check <file>
// The file (little-endian int32 throughout):
//   n_pack, then per case: length, labels[9]                                   -> a line "P word length l0 .. l8" (unpacked at 9)
//   n_trig, then per case: S, max_labels, n_target, target[n_target], and per stream: is_speech, is_active, was_speech, n_post,
//                          labels[2][max_labels], lengths[2]                   -> a line "T nf ids.. | nl ids.. | is_active.. | was_speech.."
// Before it reads the file the program holds pack / unpack / sc_scatter against their statements over every length 0..19, every
// max_labels 1..9 and seeded random label strings; it ends with "ok <n_pack> <n_trig>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "stream_ctc.h"

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)(rng_state >> 33);
}

#define CHECK(c_)                                                          \
  if (!(c_)) {                                                             \
    fprintf(stderr, "stream_ctc_check: %s failed (line %d)\n", #c_, __LINE__); \
    return 2;                                                              \
  }

static int self_check() {
  for (int rep = 0; rep < 2000; ++rep)
    for (int length = 0; length <= WW_SC_STEPS; ++length) {
      // the row ww_ctc_greedy_row leaves at max_labels 9: the first labels, the rest -1
      int32_t lab[WW_STREAM_CTC_MAX_LABELS];
      for (int i = 0; i < WW_STREAM_CTC_MAX_LABELS; ++i) lab[i] = i < length ? (int32_t)(rnd() % 7) : -1;
      const uint32_t w = ww_sc_pack(lab, length);
      CHECK((int)(w >> 27) == length);
      for (int i = 0; i < WW_STREAM_CTC_MAX_LABELS; ++i) CHECK(((w >> (3 * i)) & 7u) == (i < length ? (uint32_t)lab[i] : 0u));
      for (int m = 1; m <= WW_STREAM_CTC_MAX_LABELS; ++m) {
        std::vector<int32_t> out((size_t)m, 99);  // (exactly m entries: a write past them is the sanitizer's to see)
        CHECK(ww_sc_unpack(w, out.data(), m) == length);
        for (int i = 0; i < m; ++i) CHECK(out[(size_t)i] == (i < length ? lab[i] : -1));
      }
    }
  // sc_scatter: entries at or past n_post[s] stay as they were, in both slot orders
  for (int table = 0; table < 2; ++table)
    for (int rep = 0; rep < 200; ++rep) {
      const int S = 1 + (int)(rnd() % 5), m = 1 + (int)(rnd() % WW_STREAM_CTC_MAX_LABELS);
      std::vector<int32_t> n_post((size_t)S), labels((size_t)S * 2 * m, -77), lengths((size_t)S * 2, -77);
      std::vector<uint32_t> words((size_t)2 * S, 0xffffffffu), want;
      int nw = 0;
      for (int s = 0; s < S; ++s) {
        n_post[(size_t)s] = (int32_t)(rnd() % 3);
        for (int k = 0; k < n_post[(size_t)s]; ++k, ++nw) {
          int32_t lab[WW_STREAM_CTC_MAX_LABELS];
          const int length = (int)(rnd() % (WW_SC_STEPS + 1));
          for (int i = 0; i < WW_STREAM_CTC_MAX_LABELS; ++i) lab[i] = (int32_t)(rnd() % 7);
          const uint32_t w = ww_sc_pack(lab, length);
          words[(size_t)(table ? nw : 2 * s + k)] = w;
          want.push_back(w);
        }
      }
      sc_scatter(table != 0, S, n_post.data(), [&](int slot) { return words[(size_t)slot]; }, m, labels.data(), lengths.data());
      size_t at = 0;
      for (int s = 0; s < S; ++s)
        for (int k = 0; k < 2; ++k) {
          if (k < n_post[(size_t)s]) {
            std::vector<int32_t> out((size_t)m);
            CHECK(lengths[(size_t)s * 2 + k] == ww_sc_unpack(want[at++], out.data(), m));
            for (int i = 0; i < m; ++i) CHECK(labels[((size_t)s * 2 + k) * m + i] == out[(size_t)i]);
          } else {
            CHECK(lengths[(size_t)s * 2 + k] == -77);
            for (int i = 0; i < m; ++i) CHECK(labels[((size_t)s * 2 + k) * m + i] == -77);
          }
        }
    }
  return 0;
}

static bool rd(FILE *f, int32_t *p, size_t n) { return fread(p, 4, n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 2) return 1;
  if (int rc = self_check()) return rc;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 1;
  int32_t n_pack = 0, n_trig = 0;
  if (!rd(f, &n_pack, 1)) return 1;
  for (int c = 0; c < n_pack; ++c) {
    int32_t length, lab[WW_STREAM_CTC_MAX_LABELS], out[WW_STREAM_CTC_MAX_LABELS];
    if (!rd(f, &length, 1) || !rd(f, lab, WW_STREAM_CTC_MAX_LABELS)) return 1;
    const uint32_t w = ww_sc_pack(lab, length);
    const int32_t got = ww_sc_unpack(w, out, WW_STREAM_CTC_MAX_LABELS);
    printf("P %u %d", w, got);
    for (int i = 0; i < WW_STREAM_CTC_MAX_LABELS; ++i) printf(" %d", out[i]);
    printf("\n");
  }
  if (!rd(f, &n_trig, 1)) return 1;
  for (int c = 0; c < n_trig; ++c) {
    int32_t hd[3];
    if (!rd(f, hd, 3)) return 1;
    const int S = hd[0], m = hd[1], nt = hd[2];
    std::vector<int32_t> target((size_t)nt), n_post((size_t)S), labels((size_t)S * 2 * m), lengths((size_t)S * 2), fired((size_t)S), fall((size_t)S);
    std::vector<uint8_t> sp((size_t)S), act((size_t)S), was((size_t)S);
    if (!rd(f, target.data(), (size_t)nt)) return 1;
    for (int s = 0; s < S; ++s) {
      int32_t q[4];
      if (!rd(f, q, 4) || !rd(f, labels.data() + (size_t)s * 2 * m, (size_t)2 * m) || !rd(f, lengths.data() + (size_t)s * 2, 2)) return 1;
      sp[(size_t)s] = (uint8_t)q[0]; act[(size_t)s] = (uint8_t)q[1]; was[(size_t)s] = (uint8_t)q[2]; n_post[(size_t)s] = q[3];
    }
    if (sc_check_trigger(S, sp.data(), act.data(), labels.data(), lengths.data(), n_post.data(), m, target.data(), nt, was.data(), fired.data(),
                         &hd[0], fall.data(), &hd[1]))
      return 3;
    int32_t nf = -1, nl = -1;
    sc_trigger_update(S, sp.data(), act.data(), labels.data(), lengths.data(), n_post.data(), m, target.data(), nt, was.data(), fired.data(), &nf,
                      fall.data(), &nl);
    printf("T %d", nf);
    for (int i = 0; i < nf; ++i) printf(" %d", fired[(size_t)i]);
    printf(" | %d", nl);
    for (int i = 0; i < nl; ++i) printf(" %d", fall[(size_t)i]);
    printf(" |");
    for (int s = 0; s < S; ++s) printf(" %d", act[(size_t)s]);
    printf(" |");
    for (int s = 0; s < S; ++s) printf(" %d", was[(size_t)s]);
    printf("\n");
  }
  fclose(f);
  printf("ok %d %d\n", n_pack, n_trig);
  return 0;
}
