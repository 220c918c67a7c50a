// events_plan.h - the host-only half of ww_posterior_events / ww_posterior_events_dev (include/wwhip.h: detection events): the
// argument checks, the launch geometry and the capacity arithmetic.  Plain C++ (no HIP header, no HIP call): csrc/api.hip includes it
// for the entry points, csrc/posterior.hip for the tile size; tests/native/events_plan_check.cpp compiles it alone under Address + UB
// sanitizer on the CPU (tests/test_events_host.py).
//
// A call works on `planes` planes of n rows.  The count and write passes give every workgroup WW_EVENTS_TILE rows of one plane: the
// grid is tiles x planes, tiles = max(1, ceil(n / tile)) - one tile even for n = 0, so that a call is the same five launches whatever
// its sizes are.  The scratch, in the order ev_plan lists it, each array from a 256-byte boundary (ww_bump's rule):
//   sm        [planes][n]      fp64   the smoothed rows
//   flags     [n]              u8     bit 0: the row is its segment's first, bit 1: its last (shared by all planes)
//   offs      [n_seg + 1]      i64    the segments' row offsets ({0, n} where the caller gave none)
//   thr       [planes]         fp64
//   counts    [planes][tiles]  u32    rises per tile
//   bases     [planes][tiles]  i64    rises of the plane in front of the tile (exclusive scan)
//   totals    [planes]         i64    rises per plane
//   events    [dev_cap]        ww_event
// dev_cap = min(cap, planes * n): a plane of n rows holds at most n events (n one-row segments, all above), so no rank the write pass
// computes reaches planes * n, and ranks >= cap are never written.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/wwhip.h"

#define WW_EVENTS_TILE 256        // rows per workgroup of the count and write passes (= their threads)
#define WW_EVENTS_MAX_PLANES 64   // one wave reads all plane totals at once
#define WW_EVENTS_MAX_GRID 0x7fffffffLL
#define WW_EVENTS_PEAK_WAVES 4    // events per workgroup of the peak pass at a time (256 threads)
#define WW_EVENTS_PEAK_BLOCKS 4096  // its largest grid: a wave walks the events 4 * 4096 apart

static_assert(sizeof(ww_event) == 40, "ww_event is a fixed 40-byte record");

static inline int ev_refuse(char *err, size_t cap, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
static inline int ev_refuse(char *err, size_t cap, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  if (err && cap) vsnprintf(err, cap, fmt, ap);
  va_end(ap);
  return WW_EINVAL;
}

// tiles of n rows: at least one (see above).  n >= 0.
static inline int64_t ev_tiles(int64_t n) { return n <= 0 ? 1 : (n - 1) / WW_EVENTS_TILE + 1; }

// events the call writes to the caller's array: the first min(total, cap) in (plane, segment, start) order
static inline int64_t ev_written(int64_t total, int64_t cap) { return total < cap ? total : cap; }

// events the device buffer has room for: min(cap, planes * n) (planes <= 64 and n <= 2^48: no overflow)
static inline int64_t ev_dev_cap(int64_t n, int64_t planes, int64_t cap) {
  const int64_t most = planes * n;
  return cap < most ? cap : most;
}

// The arguments of ww_posterior_events[_dev] (include/wwhip.h lists the refusals): WW_OK, or WW_EINVAL with the reason in err.
// `post` is the host or device plane pointer - only looked at for NULL.
static inline int ev_check(const void *post, int64_t n, int64_t planes, const int64_t *seg_offs, int64_t n_seg, const double *thr,
                           const void *events, int64_t cap, const void *n_events, char *err, size_t ecap) {
  if (planes < 1 || planes > WW_EVENTS_MAX_PLANES) return ev_refuse(err, ecap, "%lld planes: a call takes 1..%d", (long long)planes, WW_EVENTS_MAX_PLANES);
  if (n < 0) return ev_refuse(err, ecap, "negative row count %lld", (long long)n);
  if (n_seg < 0) return ev_refuse(err, ecap, "negative segment count %lld", (long long)n_seg);
  if (cap < 0) return ev_refuse(err, ecap, "negative event capacity %lld", (long long)cap);
  if (!thr) return ev_refuse(err, ecap, "NULL thresholds");
  if (!n_events) return ev_refuse(err, ecap, "NULL n_events");
  if (!events && cap > 0) return ev_refuse(err, ecap, "NULL events with room for %lld", (long long)cap);
  if (!post && n > 0) return ev_refuse(err, ecap, "NULL posteriors with %lld rows", (long long)n);
  if (n > (int64_t)1 << 48) return ev_refuse(err, ecap, "%lld rows: more than a call can address", (long long)n);
  if (seg_offs) {
    for (int64_t u = 0; u <= n_seg; ++u) {
      if (seg_offs[u] < 0 || seg_offs[u] > n)
        return ev_refuse(err, ecap, "seg_offs[%lld] = %lld outside [0, %lld]", (long long)u, (long long)seg_offs[u], (long long)n);
      if (u && seg_offs[u] < seg_offs[u - 1])
        return ev_refuse(err, ecap, "seg_offs[%lld] = %lld descends from %lld", (long long)u, (long long)seg_offs[u], (long long)seg_offs[u - 1]);
    }
  }
  return WW_OK;
}

struct ev_plan {
  int64_t n = 0, tiles = 1, n_offs = 2, dev_cap = 0;
  int32_t planes = 1;
  int64_t peak_blocks = 1;
  // byte offsets of the scratch arrays inside one allocation of `bytes`
  size_t o_sm = 0, o_flags = 0, o_offs = 0, o_thr = 0, o_counts = 0, o_bases = 0, o_totals = 0, o_events = 0, bytes = 0;
};

static inline size_t ev_round(size_t b) { return (b + 255) & ~(size_t)255; }

// Geometry and scratch of a checked call (ev_check passed).  n_seg counts the caller's segments; has_offs = it gave offsets.  WW_EINVAL
// (the plan is filled in all the same) where the tiles do not fit one launch.
static inline int ev_make_plan(int64_t n, int32_t planes, bool has_offs, int64_t n_seg, int64_t cap, ev_plan &p, char *err, size_t ecap) {
  p.n = n;
  p.planes = planes;
  p.tiles = ev_tiles(n);
  p.n_offs = has_offs ? n_seg + 1 : 2;
  p.dev_cap = ev_dev_cap(n, planes, cap);
  const int64_t per = WW_EVENTS_PEAK_WAVES;
  p.peak_blocks = p.dev_cap <= 0 ? 1 : (p.dev_cap - 1) / per + 1;
  if (p.peak_blocks > WW_EVENTS_PEAK_BLOCKS) p.peak_blocks = WW_EVENTS_PEAK_BLOCKS;
  size_t o = 0;
  p.o_sm = o;
  o += ev_round((size_t)planes * (size_t)n * 8 + 8);
  p.o_flags = o;
  o += ev_round((size_t)n + 1);
  p.o_offs = o;
  o += ev_round((size_t)p.n_offs * 8);
  p.o_thr = o;
  o += ev_round((size_t)planes * 8);
  p.o_counts = o;
  o += ev_round((size_t)planes * (size_t)p.tiles * 4);
  p.o_bases = o;
  o += ev_round((size_t)planes * (size_t)p.tiles * 8);
  p.o_totals = o;
  o += ev_round((size_t)planes * 8);
  p.o_events = o;
  o += ev_round((size_t)p.dev_cap * sizeof(ww_event) + sizeof(ww_event));
  p.bytes = o;
  if (p.tiles > WW_EVENTS_MAX_GRID) return ev_refuse(err, ecap, "%lld rows are %lld tiles: more than one launch takes", (long long)n, (long long)p.tiles);
  return WW_OK;
}
