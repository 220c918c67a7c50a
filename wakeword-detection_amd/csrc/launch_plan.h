// launch_plan.h - the host-only half of every call that builds a launch table: the descriptor structs the kernels read (one per
// workgroup), the constants their planners share with the kernels, the planners themselves (pure integer arithmetic on the
// caller's offset arrays) and the layout of a call's tables in one block.  Plain C++ (no HIP header, no HIP call): common.h
// includes it for the .hip files, and tests/native/launch_plan_check.cpp compiles it alone under Address + UB sanitizer on the CPU
// (tests/test_host_logic.py).  How a block reaches the device is ww_tables::send (common.h).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/wwhip.h"

#define WW_NUM_CUS 256  // MI355X (gfx950): 8 XCDs x 32 CUs

// bump allocator over the ctx workspace
struct ww_bump {
  char *base;
  size_t off = 0, cap;
  ww_bump(void *p, size_t c) : base((char *)p), cap(c) {}
  template <typename T>
  T *take(size_t n) {
    size_t bytes = (n * sizeof(T) + 255) & ~size_t(255);
    T *r = (T *)(base + off);
    off += bytes;
    return r;
  }
  static size_t need(size_t n, size_t elem) { return (n * elem + 255) & ~size_t(255); }
};

// The launch tables of one call as ONE block: add() registers them in order, each from a 256-byte boundary - ww_bump::take's rule,
// so the block is what a ww_bump over the same counts hands out and bytes() is the sum of their ww_bump::need.  join() lengthens the
// table before it (lists of one element type that a kernel indexes as one).  An empty table (nullptr, 0) costs nothing.  The
// arrays are only read by pack(): they must live until then and no longer.
struct ww_table_block {
  struct entry {
    const void *src;
    size_t bytes, off;
  };
  std::vector<entry> tabs;
  size_t used = 0;  // end of the last table's bytes
  size_t bytes() const { return (used + 255) & ~size_t(255); }
  template <typename T>
  size_t add(const T *p, size_t n) {  // -> the table's offset in the block
    tabs.push_back({p, n * sizeof(T), bytes()});
    used = tabs.back().off + n * sizeof(T);
    return tabs.back().off;
  }
  template <typename T>
  void join(const T *p, size_t n) {
    tabs.push_back({p, n * sizeof(T), used});
    used += n * sizeof(T);
  }
  template <typename T>
  size_t add(const std::vector<T> &v) { return add(v.data(), v.size()); }
  template <typename T>
  void join(const std::vector<T> &v) { join(v.data(), v.size()); }
  void pack(void *dst) const {  // bytes() bytes: the tables, zeros between and behind them
    size_t at = 0;
    for (const entry &e : tabs) {
      if (e.off > at) memset((char *)dst + at, 0, e.off - at);
      if (e.bytes) memcpy((char *)dst + e.off, e.src, e.bytes);
      at = e.off + e.bytes;
    }
    if (bytes() > at) memset((char *)dst + at, 0, bytes() - at);
  }
};

// ---- the CRNN's sliding form (crnn.hip: crnn_rows_kernel, gru_tail_kernel) ------------------------------------------------------
struct rows_tile {
  int64_t start;    // mel row of the tile's first field
  int64_t out_row;  // row of out[kind] its first position goes to
  int32_t stride, count, kind, pad;
};

// interior fields lie at stride g = gcd(hop, 8) rows; nw windows at `hop` need n_int of them
static inline int crnn_gcd8(int hop) { return hop % 8 == 0 ? 8 : hop % 4 == 0 ? 4 : hop % 2 == 0 ? 2 : 1; }
static inline int64_t crnn_n_int(int64_t nw, int hop) { return ((nw - 1) * hop + 128) / crnn_gcd8(hop) + 1; }

// ---- a segments call's descriptors (ww_forward_segments_dev, ww_set_forward_segments_dev): sequence s is seg_nw[s] windows of T
// rows at seg_row0[s] + k * hop, all inside the mel buffer ------------------------------------------------------------------------
#define WW_SEG_ERR 96  // room for the text of a refusal
// sequence s alone: WW_OK, or WW_EINVAL with the reason in err
static inline int seg_check(const int64_t *seg_row0, const int32_t *seg_nw, int s, int hop, int T, int64_t mel_rows, char *err) {
  const int nw = seg_nw[s];
  if (nw < 0) {
    snprintf(err, WW_SEG_ERR, "negative window count in sequence %d", s);
    return WW_EINVAL;
  }
  if (nw && (seg_row0[s] < 0 || seg_row0[s] + (int64_t)(nw - 1) * hop + T > mel_rows)) {
    snprintf(err, WW_SEG_ERR, "sequence %d: windows leave the mel buffer", s);
    return WW_EINVAL;
  }
  return WW_OK;
}
// the whole call, before anything is enqueued: *W = its windows, or the first fault
static inline int seg_walk(const int64_t *seg_row0, const int32_t *seg_nw, int n_seg, int hop, int T, int64_t mel_rows, int64_t *W, char *err) {
  *W = 0;
  for (int s = 0; s < n_seg; ++s) {
    if (int rc = seg_check(seg_row0, seg_nw, s, hop, T, mel_rows, err)) return rc;
    *W += seg_nw[s];
  }
  return WW_OK;
}
// a checked call's windows as an explicit list of start rows, appended sequence by sequence
static inline void seg_rows(const int64_t *seg_row0, const int32_t *seg_nw, int n_seg, int hop, std::vector<int64_t> &rows) {
  for (int s = 0; s < n_seg; ++s)
    for (int k = 0; k < seg_nw[s]; ++k) rows.push_back(seg_row0[s] + (int64_t)k * hop);
}

// groups of whole sequences of at most ~WW_SEG_GROUP windows bound the workspace (a model set's call: windows x members of the call,
// its cap per member is WW_SEG_GROUP / members)
#define WW_SEG_GROUP 32768

// One group of ww_k_crnn_segments_forward: sequences [s0, next) of the call, nW windows numbered sequence by sequence and nI
// interior fields; crnn_rows_kernel's tiles (no tile straddles two sequences) and each window's first interior field.  `cap`: the
// group takes sequences while its windows stay at or below it (its first sequence whatever its size).  Tiles and i0 are functions
// of the sequences alone: where the cap cuts only moves the group's bases (nI, nW so far) under them.
struct crnn_seg_group {
  std::vector<rows_tile> tiles;
  std::vector<int64_t> i0;
  int64_t nI = 0, nW = 0;
  int next = 0;
  char err[WW_SEG_ERR] = {0};  // why planning stopped (status != WW_OK), for ww_fail
};
static inline int crnn_plan_group(const int64_t *seg_row0, const int32_t *seg_nw, int n_seg, int hop, int T, int PT, int OT, int ST,
                                  int64_t mel_rows, int s0, crnn_seg_group &gp, int64_t cap = WW_SEG_GROUP) {
  const int g = crnn_gcd8(hop);
  gp.tiles.clear();
  gp.i0.clear();
  int64_t nI = 0, nW = 0;
  int s1 = s0;
  for (; s1 < n_seg && (s1 == s0 || nW + seg_nw[s1] <= cap); ++s1) {
    if (int rc = seg_check(seg_row0, seg_nw, s1, hop, T, mel_rows, gp.err)) return rc;
    const int nw = seg_nw[s1];
    if (nw == 0) continue;
    const int64_t r0 = seg_row0[s1];
    const int64_t n_int = crnn_n_int(nw, hop);
    for (int64_t p0 = 0; p0 < n_int; p0 += 16)
      gp.tiles.push_back({r0 + 2 + (int64_t)g * p0, nI + p0, g, (int32_t)(n_int - p0 < 16 ? n_int - p0 : 16), 0, 0});
    for (int p0 = 0; p0 < nw; p0 += 16) {
      const int32_t cnt = nw - p0 < 16 ? nw - p0 : 16;
      gp.tiles.push_back({r0 - PT + (int64_t)hop * p0, nW + p0, hop, cnt, 1, 0});
      gp.tiles.push_back({r0 + (int64_t)(OT - 1) * ST - PT + (int64_t)hop * p0, nW + p0, hop, cnt, 2, 0});
    }
    for (int k = 0; k < nw; ++k) gp.i0.push_back(nI + (int64_t)k * hop / g);
    nI += n_int;
    nW += nw;
  }
  gp.nI = nI;
  gp.nW = nW;
  gp.next = s1;
  return WW_OK;
}

// ---- the Wavenet's sequence form (wavenet.hip: wavenet_seq_kernel) ---------------------------------------------------------------
// A segment = rows [row0, row0 + n) of the mel buffer, all of one sequence; outputs of its first `skip` rows (the warm-up of a
// segment that does not start at its sequence's row 0) are discarded.
struct wv_seg {
  int64_t row0;
  int32_t n, skip;
};
// The library's segment length for `rows` rows of work (WW_OPT_WAVE_SEQ_SEGMENT = 0), for ww_wave_sequence and the stream feed
// alike; each clamps it to what its cuts need.  A segment's warm-up (rf - 1 rows) + its rows are a whole number of 192-row chunks:
// about two segments per CU once there is enough work, 10 chunks at least (warm-up: a tenth of the rows at most) and 64 at most.
static inline int64_t ww_wave_segment_rows(int64_t rows, int rf) {
  int64_t chunks = (rows + 2 * WW_NUM_CUS * 192 - 1) / (2 * WW_NUM_CUS * 192);
  chunks = chunks < 10 ? 10 : chunks > 64 ? 64 : chunks;
  return chunks * 192 - (rf - 1);
}

// Device scratch of one call: the segment table, the device copy of row_offs, logits where the caller wants none, and the two
// buffers of the pooled maximum - `planes` planes of total_rows rows each.  A model set's call adds its member ids and, where each
// sequence has a member of its own, seg_seq: the sequence of segment i - a table BESIDE the segments, wv_seg stays as it is.
struct wave_seq_plan {
  std::vector<wv_seg> segs;
  std::vector<int32_t> seg_seq;
  int64_t max_len = 0;
  size_t b_segs = 0, b_offs = 0, b_z = 0, b_pool = 0, b_ids = 0, b_aux = 0;
  size_t bytes() const { return b_segs + b_offs + b_ids + b_aux + b_z + 2 * b_pool; }
};
// How a call names its members.  NONE: a single model (one plane, no table).  BY_PLANE: plane k by member ids[k], `planes` ids - the
// plane is a grid dimension and there is no second table.  BY_SEQ: one plane, sequence s by member ids[s], n_seq ids - a segment
// finds its member through seg_seq, written as the cuts are made (empty sequences have no segment).
enum wave_seq_ids { WAVE_SEQ_IDS_NONE, WAVE_SEQ_IDS_BY_PLANE, WAVE_SEQ_IDS_BY_SEQ };
// Cuts: a sequence is computed in segments of G rows; every segment but a sequence's first starts RF - 1 rows early and drops them.
// G = seg_opt (WW_OPT_WAVE_SEQ_SEGMENT), or if that is 0 the library's: ww_wave_segment_rows', at least one chunk.  The cuts are the
// same for every plane and every id form: a member is weights, not geometry.
static inline void wave_seq_make_plan(int rf, int n_out, int64_t seg_opt, int64_t total_rows, const int64_t *row_offs, int n_seq, int planes,
                                      wave_seq_ids ids, bool need_z, bool need_pool, wave_seq_plan &pl) {
  int64_t span = 0;
  for (int s = 0; s < n_seq; ++s) {
    span += row_offs[s + 1] - row_offs[s];
    pl.max_len = std::max<int64_t>(pl.max_len, row_offs[s + 1] - row_offs[s]);
  }
  int64_t G = seg_opt;
  if (G <= 0) G = std::max<int64_t>(ww_wave_segment_rows(span, rf), 192);
  for (int s = 0; s < n_seq; ++s) {
    const int64_t o = row_offs[s], len = row_offs[s + 1] - o;
    for (int64_t s0 = 0; s0 < len; s0 += G) {
      const int64_t warm = std::min<int64_t>(s0, rf - 1), rows = std::min<int64_t>(G, len - s0);
      pl.segs.push_back({o + s0 - warm, (int32_t)(warm + rows), (int32_t)warm});
      if (ids == WAVE_SEQ_IDS_BY_SEQ) pl.seg_seq.push_back(s);
    }
  }
  const size_t rows = (size_t)planes * (size_t)total_rows * n_out;
  pl.b_segs = ww_bump::need(pl.segs.size(), sizeof(wv_seg));
  pl.b_offs = ww_bump::need((size_t)n_seq + 1, 8);
  pl.b_z = need_z ? ww_bump::need(rows, 4) : 0;
  pl.b_pool = need_pool ? ww_bump::need(rows, 4) : 0;
  pl.b_ids = ids == WAVE_SEQ_IDS_NONE ? 0 : ww_bump::need(ids == WAVE_SEQ_IDS_BY_SEQ ? (size_t)n_seq : (size_t)planes, 4);
  pl.b_aux = ww_bump::need(pl.seg_seq.size(), 4);
}

// ---- a causal bank's feed (streams.hip: ww_stream_feed) ---------------------------------------------------------------------------
#define FEED_GROUP 16          // new frames of one stream per workgroup of stream_feed_frontend_kernel
#define WV_FEED_HIST_ROWS 16   // rows of BatchNorm output a block carries (wavenet.hip: WV_PAD)
#define WW_FEED_TILE_ROWS 16   // up to here a stream's new rows are one tile of the one-wave form, tail included
#define WW_FEED_POOL_ROWS 256  // rows per workgroup of wave_feed_pool_kernel
struct feed_str {       // a stream of the call
  int64_t s_off;        // its packet's first sample in the call's sample buffer
  int64_t k;            // samples in the packet
  int64_t r_off;        // its first new row in the call's row buffer
  int32_t sid, fill, rows, pos;
};
struct feed_grp {
  int32_t i, f0, nf, pad;  // stream of the call, first frame, frames (0: the stream's state only)
};
// The sequence form over the rows a call brought, stream by stream.  A segment is rows [row0, row0 + n) of the call's row buffer,
// all of one stream; bit 0 of flags: its history comes from the stream's state (the stream's first segment; the others start
// RF - 1 rows early from zeros and drop `skip` rows), bit 1: its history goes back there (the stream's last segment).
struct wv_feed_seg {
  int64_t row0;
  int32_t n, skip, sid, flags;
};
// the pooled maxima of a stream that brought more rows than one tile: rows [k0, k0 + 256) of its n new rows, which start at row0
struct wv_feed_pool {
  int64_t row0;
  int32_t n, sid, k0, pad;
};

// The cuts of a stream that brought more rows than one tile.  Segments of G rows as ww_wave_sequence cuts them,
// with two differences: a segment that is not the stream's first needs its whole warm-up inside the call's row buffer (the rows in
// front of the call's first row are gone), hence G >= RF - 1; and the stream's history is taken from its last segment, whose 16
// rows per block are the uncut evaluation's only after RF - 1 + 16 rows from zeros: a last segment that keeps fewer than 16 rows
// is merged into the one before it.
static inline void feed_cut(std::vector<wv_feed_seg> &segs, int64_t r_off, int64_t rows, int sid, int64_t G, int rf) {
  for (int64_t s0 = 0; s0 < rows; s0 += G) {
    int64_t len = std::min<int64_t>(G, rows - s0);
    if (rows - (s0 + len) < WV_FEED_HIST_ROWS && rows - (s0 + len) > 0) len = rows - s0;  // (the next one would be too short to carry the history)
    const int64_t warm = s0 ? rf - 1 : 0;
    segs.push_back({r_off + s0 - warm, (int32_t)(warm + len), (int32_t)warm, sid, s0 ? 0 : 1});
    if (s0 + len >= rows) break;
  }
  segs.back().flags |= 2;
}

// The plan of a feed: streams, front-end groups, model segments (one-wave form: small; twelve-wave form: large), the twelve-wave
// form's tail.  ids / sample_offs / row_offs are the call's (row_offs as feed_check left them); fill / pos are the bank's, by stream id.
struct feed_plan {
  std::vector<feed_str> str;
  std::vector<feed_grp> grp;
  std::vector<wv_feed_seg> small, large;
  std::vector<wv_feed_pool> pool, ringt;
};
static inline void feed_make_plan(const int32_t *ids, int n, const int64_t *sample_offs, const int64_t *row_offs, const int *fill, const int *pos,
                                  int T, int rf, int64_t seg_opt, feed_plan &pl) {
  pl.str.resize((size_t)n);
  int64_t large_rows = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t r = row_offs[i + 1] - row_offs[i];
    if (r > WW_FEED_TILE_ROWS || r > T) large_rows += r;
  }
  int64_t G = seg_opt;
  if (G <= 0) G = ww_wave_segment_rows(large_rows, rf);
  G = std::min<int64_t>(std::max<int64_t>(G, std::max(rf - 1, 1)), 1 << 30);
  for (int i = 0; i < n; ++i) {
    const int s = ids[i];
    const int64_t k = sample_offs[i + 1] - sample_offs[i], r = row_offs[i + 1] - row_offs[i];
    pl.str[i] = {sample_offs[i] - sample_offs[0], k, row_offs[i], s, fill[s], (int32_t)r, pos[s]};
    if (k == 0) continue;  // an empty packet: the stream stands still
    if (r == 0) pl.grp.push_back({i, 0, 0, 0});
    for (int64_t f0 = 0; f0 < r; f0 += FEED_GROUP) pl.grp.push_back({i, (int32_t)f0, (int32_t)std::min<int64_t>(FEED_GROUP, r - f0), 0});
    if (r == 0) continue;
    if (r <= WW_FEED_TILE_ROWS && r <= T) {
      pl.small.push_back({row_offs[i], (int32_t)r, 0, s, 3});
    } else {
      feed_cut(pl.large, row_offs[i], r, s, G, rf);
      for (int64_t k0 = 0; k0 < r; k0 += WW_FEED_POOL_ROWS) pl.pool.push_back({row_offs[i], (int32_t)r, s, (int32_t)k0, 0});
      pl.ringt.push_back({row_offs[i], (int32_t)r, s, 0, 0});
    }
  }
}

// The same plan for a bank of K member slots per stream (ww_stream_feed_all): streams, groups and segments stay the physical streams'
// - the sequence kernel's every-member form runs a segment once per slot and finds the virtual stream itself.  The tail's kernels are
// the single bank's, so their tables are written out per slot: slot j's entry names virtual stream sid K + j, and rows of plane j of
// the logits and posteriors ([K][rows] rows: row0 + j rows), entry by entry in slot order.
static inline void feed_plan_all(feed_plan &pl, int K, int64_t rows) {
  auto per_slot = [&](std::vector<wv_feed_pool> &t) {
    std::vector<wv_feed_pool> out;
    out.reserve(t.size() * (size_t)K);
    for (const wv_feed_pool &d : t)
      for (int j = 0; j < K; ++j) out.push_back({d.row0 + (int64_t)j * rows, d.n, d.sid * K + j, d.k0, 0});
    t.swap(out);
  };
  per_slot(pl.pool);
  per_slot(pl.ringt);
}

// ---- the resampler (resample.hip) ------------------------------------------------------------------------------------------------
#define RS_XCAP WW_RESAMPLE_MAX_SPAN  // floats of staged input per tile (48 KB: three workgroups per CU)
#define RS_R 8                        // outputs per item, phase form
#define RS_R1 7                       // outputs per lane, up == 1 form: odd, so that the lane stride RS_R1 * down keeps odd `down` conflict-free
#define RS_COPY 4096                  // outputs per tile of the identity form

struct rs_tile {
  int64_t in_off;     // index in the input buffer of the segment's first sample
  int64_t in_first;   // absolute index of that sample in its signal
  int64_t n_in;       // samples of the segment
  int64_t out_off;    // index in the output buffer of output out_first
  int64_t out_first;  // absolute index of the segment's first output
  int64_t out_end;    // one past its last
  int64_t k_lo;       // absolute index of staged sample 0
  int64_t first;      // phase form: first item; up == 1 and identity forms: first output
  int32_t n_x;        // staged samples (<= RS_XCAP)
  int32_t n;          // phase form: items; up == 1 form: lanes; identity form: outputs
};

// what the plan needs of a resampler (ww_resampler extends it)
struct rs_geom {
  int64_t up = 1, down = 1, half = 0, tpp = 0;
  bool identity = false;
  int32_t n_u = 0;          // up == 1: rows of the tap table d_h2 (a multiple of RS_UNROLL1)
  int32_t lanes1 = 0;       // up == 1 form: lanes per tile (0: the form does not fit, the phase form runs)
  int32_t ne8 = 0, ne1 = 0; // phase form: items per tile for R = 8 (0: does not fit) and R = 1
};

static inline int64_t rs_out_len(const rs_geom *r, int64_t n) {  // ceil(n * up / down)
  return (int64_t)(((__int128)n * r->up + r->down - 1) / r->down);
}

// worst-case staged samples of a phase-form tile of ne items
static inline int64_t rs_phase_span(const rs_geom *r, int R, int64_t ne) {
  const int64_t nA = (ne - 1) / r->up + 2;
  return nA * R * r->down + r->tpp + 2;
}

struct rs_plan {
  std::vector<rs_tile> copy, decim, ph8, ph1;
  size_t count() const { return copy.size() + decim.size() + ph8.size() + ph1.size(); }
};

static inline void rs_plan_phase(const rs_geom *r, int R, int64_t ne, rs_tile base, std::vector<rs_tile> &dst) {
  const int64_t up = r->up, down = r->down, J = r->half / up, Jmin = (r->half - up + 1) / up;
  const int64_t e_lo = ((base.out_first / up) / R) * up, e_hi = (((base.out_end - 1) / up) / R + 1) * up;
  for (int64_t e0 = e_lo; e0 < e_hi; e0 += ne) {
    const int64_t n = std::min(ne, e_hi - e0), A0 = e0 / up, A1 = (e0 + n - 1) / up;
    rs_tile t = base;
    t.first = e0;
    t.n = (int32_t)n;
    t.k_lo = A0 * R * down - J;
    t.n_x = (int32_t)((A1 * R + R - 1) * down + (down - 1) - Jmin + r->tpp - t.k_lo);
    dst.push_back(t);
  }
}

static inline int rs_make_plan(const rs_geom *r, const int64_t *so, const int64_t *in_first, const int64_t *out_first, const int64_t *oo,
                               int n_seg, rs_plan &pl) {
  for (int u = 0; u < n_seg; ++u) {
    const int64_t cnt = oo[u + 1] - oo[u];
    if (cnt <= 0) continue;
    rs_tile b = {};
    b.in_off = so[u];
    b.in_first = in_first ? in_first[u] : 0;
    b.n_in = so[u + 1] - so[u];
    b.out_off = oo[u];
    b.out_first = out_first ? out_first[u] : 0;
    b.out_end = b.out_first + cnt;
    if (r->identity) {
      for (int64_t m = b.out_first; m < b.out_end; m += RS_COPY) {
        rs_tile t = b;
        t.first = m;
        t.n = (int32_t)std::min<int64_t>(RS_COPY, b.out_end - m);
        pl.copy.push_back(t);
      }
    } else if (r->up == 1 && r->lanes1 > 0) {
      const int64_t per = (int64_t)r->lanes1 * RS_R1;
      for (int64_t m = b.out_first; m < b.out_end; m += per) {
        rs_tile t = b;
        t.first = m;
        t.n = (int32_t)std::min<int64_t>(r->lanes1, (b.out_end - m + RS_R1 - 1) / RS_R1);
        t.k_lo = m * r->down - r->half;
        t.n_x = (int32_t)((int64_t)(t.n - 1) * RS_R1 * r->down + r->n_u);
        pl.decim.push_back(t);
      }
    } else if (r->ne8 > 0 && cnt >= 2 * RS_R * r->up) {
      rs_plan_phase(r, RS_R, r->ne8, b, pl.ph8);
    } else {
      rs_plan_phase(r, 1, r->ne1, b, pl.ph1);
    }
  }
  return WW_OK;
}
