// events_plan_check - the host-only half of ww_posterior_events (csrc/events_plan.h: argument checks, launch geometry, capacity
// arithmetic) alone on the CPU, under Address + UB sanitizer (tests/test_events_host.py compiles and runs it; nothing here touches a
// GPU):
//   * every refusal include/wwhip.h lists - planes outside 1..64, negative n / n_seg / cap, descending offsets, offsets outside [0, n],
//     NULL thr, NULL n_events, NULL events with cap > 0, NULL posteriors with rows - each with its reason, and the calls next to them
//     that are accepted (cap = 0 with NULL events, n = 0, empty segments, no offsets at all);
//   * the tiles of n = 0, 1, tile - 1, tile, tile + 1, 3 tile + 7 and 2^40 rows, and that every row lies in exactly one tile;
//   * the capacity arithmetic: dev_cap = min(cap, planes * n), ev_written = min(total, cap), the peak pass's grid, no overflow at 2^40
//     rows x 64 planes; the 2^40-row plan is computed and then refused for its grid (2^32 tiles are more than one launch takes);
//   * the scratch layout: arrays in order, 256-byte aligned, disjoint, each large enough for what the kernels index.
// Prints "ok <checks>" and exits 0; or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "events_plan.h"

static long n_checks = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    ++n_checks;                                                                \
    if (!(cond)) {                                                             \
      fprintf(stderr, "events_plan_check: %s (line %d)\n", #cond, __LINE__);  \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

static char err[256];
static int check(const void *post, int64_t n, int64_t planes, const int64_t *offs, int64_t n_seg, const double *thr, const void *events, int64_t cap,
                 const void *n_events) {
  memset(err, 0, sizeof err);
  return ev_check(post, n, planes, offs, n_seg, thr, events, cap, n_events, err, sizeof err);
}
static bool says(const char *what) { return strstr(err, what) != nullptr; }

static void refusals() {
  float post[8] = {0};
  double thr[64] = {0};
  ww_event ev[4];
  int64_t n_ev = 0;
  const int64_t ok_offs[4] = {0, 3, 3, 8}, desc[4] = {0, 5, 4, 8}, past[3] = {0, 4, 9}, neg[3] = {-1, 4, 8};
  CHECK(check(post, 8, 1, nullptr, 0, thr, ev, 4, &n_ev) == WW_OK && err[0] == 0);
  CHECK(check(post, 8, 64, ok_offs, 3, thr, ev, 4, &n_ev) == WW_OK);
  CHECK(check(post, 8, 1, ok_offs, 0, thr, ev, 4, &n_ev) == WW_OK);       // no segment at all: one offset is read
  CHECK(check(post, 8, 1, nullptr, 0, thr, nullptr, 0, &n_ev) == WW_OK);  // count only
  CHECK(check(nullptr, 0, 1, nullptr, 0, thr, nullptr, 0, &n_ev) == WW_OK);
  for (int64_t planes : {0, -1, 65, 1000}) CHECK(check(post, 8, planes, nullptr, 0, thr, ev, 4, &n_ev) == WW_EINVAL && says("planes"));
  CHECK(check(post, -1, 1, nullptr, 0, thr, ev, 4, &n_ev) == WW_EINVAL && says("negative row count"));
  CHECK(check(post, 8, 1, ok_offs, -1, thr, ev, 4, &n_ev) == WW_EINVAL && says("negative segment count"));
  CHECK(check(post, 8, 1, nullptr, -1, thr, ev, 4, &n_ev) == WW_EINVAL && says("negative segment count"));
  CHECK(check(post, 8, 1, nullptr, 0, thr, ev, -1, &n_ev) == WW_EINVAL && says("negative event capacity"));
  CHECK(check(post, 8, 1, desc, 3, thr, ev, 4, &n_ev) == WW_EINVAL && says("descends"));
  CHECK(check(post, 8, 1, past, 2, thr, ev, 4, &n_ev) == WW_EINVAL && says("outside"));
  CHECK(check(post, 8, 1, neg, 2, thr, ev, 4, &n_ev) == WW_EINVAL && says("outside"));
  CHECK(check(post, 8, 1, nullptr, 0, nullptr, ev, 4, &n_ev) == WW_EINVAL && says("NULL thresholds"));
  CHECK(check(post, 8, 1, nullptr, 0, thr, ev, 4, nullptr) == WW_EINVAL && says("NULL n_events"));
  CHECK(check(post, 8, 1, nullptr, 0, thr, nullptr, 1, &n_ev) == WW_EINVAL && says("NULL events"));
  CHECK(check(nullptr, 8, 1, nullptr, 0, thr, ev, 4, &n_ev) == WW_EINVAL && says("NULL posteriors"));
  CHECK(check(post, ((int64_t)1 << 48) + 1, 1, nullptr, 0, thr, ev, 4, &n_ev) == WW_EINVAL && says("more than a call can address"));
  CHECK(ev_refuse(nullptr, 0, "x") == WW_EINVAL);  // no room for a reason is no crash
}

static void tiles_and_capacity() {
  const int64_t T = WW_EVENTS_TILE, big = (int64_t)1 << 40;
  CHECK(T == 256);
  CHECK(ev_tiles(0) == 1 && ev_tiles(1) == 1 && ev_tiles(T - 1) == 1 && ev_tiles(T) == 1 && ev_tiles(T + 1) == 2);
  CHECK(ev_tiles(3 * T + 7) == 4 && ev_tiles(414000) == 1618 && ev_tiles(big) == (int64_t)1 << 32);
  for (int64_t n : {(int64_t)1, T - 1, T, T + 1, 3 * T + 7, big}) {  // the last row lies in the last tile, and the tile before does not reach it
    CHECK((n - 1) / T == ev_tiles(n) - 1);
    CHECK((ev_tiles(n) - 1) * T < n && ev_tiles(n) * T >= n);
  }
  CHECK(ev_written(0, 0) == 0 && ev_written(7, 0) == 0 && ev_written(7, 1) == 1 && ev_written(7, 6) == 6 && ev_written(7, 7) == 7 && ev_written(7, 12) == 7);
  CHECK(ev_dev_cap(0, 64, 100) == 0 && ev_dev_cap(10, 3, 100) == 30 && ev_dev_cap(10, 3, 29) == 29 && ev_dev_cap(10, 3, 0) == 0);
  CHECK(ev_dev_cap(big, 64, INT64_MAX) == (int64_t)1 << 46 && ev_dev_cap(big, 64, 5) == 5);

  for (int64_t n : {(int64_t)0, (int64_t)1, T - 1, T, T + 1, 3 * T + 7, (int64_t)414000})
    for (int planes : {1, 3, 64})
      for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)1000, INT64_MAX})
        for (int has : {0, 1}) {
          ev_plan p;
          const int64_t n_seg = 200;
          CHECK(ev_make_plan(n, planes, has != 0, n_seg, cap, p, err, sizeof err) == WW_OK);
          CHECK(p.n == n && p.planes == planes && p.tiles == ev_tiles(n) && p.n_offs == (has ? n_seg + 1 : 2));
          CHECK(p.dev_cap == (cap < planes * n ? cap : planes * n));
          CHECK(p.peak_blocks >= 1 && p.peak_blocks <= WW_EVENTS_PEAK_BLOCKS);
          CHECK(p.peak_blocks == WW_EVENTS_PEAK_BLOCKS || p.peak_blocks * WW_EVENTS_PEAK_WAVES >= p.dev_cap);
          const size_t o[9] = {p.o_sm, p.o_flags, p.o_offs, p.o_thr, p.o_counts, p.o_bases, p.o_totals, p.o_events, p.bytes};
          const size_t need[8] = {(size_t)planes * n * 8, (size_t)n, (size_t)p.n_offs * 8, (size_t)planes * 8, (size_t)planes * p.tiles * 4,
                                  (size_t)planes * p.tiles * 8, (size_t)planes * 8, (size_t)p.dev_cap * sizeof(ww_event)};
          CHECK(o[0] == 0);
          for (int k = 0; k < 8; ++k) CHECK(o[k] % 256 == 0 && o[k + 1] >= o[k] + need[k]);
        }
  ev_plan p;
  CHECK(ev_make_plan(big, 64, false, 0, INT64_MAX, p, err, sizeof err) == WW_EINVAL && says("more than one launch takes"));
  CHECK(p.tiles == (int64_t)1 << 32 && p.dev_cap == (int64_t)1 << 46 && p.peak_blocks == WW_EVENTS_PEAK_BLOCKS);
  CHECK(p.o_flags >= ((size_t)1 << 49) && p.bytes > p.o_events && p.bytes - p.o_events >= ((size_t)40 << 46));
  CHECK(ev_make_plan(WW_EVENTS_MAX_GRID * T, 1, false, 0, 0, p, err, sizeof err) == WW_OK && p.tiles == WW_EVENTS_MAX_GRID);
  CHECK(ev_make_plan(WW_EVENTS_MAX_GRID * T + 1, 1, false, 0, 0, p, err, sizeof err) == WW_EINVAL);
}

int main() {
  CHECK(sizeof(ww_event) == 40);
  ww_event e;
  CHECK((char *)&e.seg - (char *)&e == 4 && (char *)&e.start - (char *)&e == 8 && (char *)&e.end - (char *)&e == 16 &&
        (char *)&e.peak - (char *)&e == 24 && (char *)&e.peak_value - (char *)&e == 32);
  refusals();
  tiles_and_capacity();
  printf("ok %ld\n", n_checks);
  return 0;
}
