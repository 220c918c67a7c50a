// launch_plan_check - csrc/launch_plan.h alone on the CPU, under Address + UB sanitizer (tests/test_host_logic.py): the table
// block's layout against ww_bump, and every planner's output against the properties the kernels rely on, over a fixed seed.
// Prints "ok <checks>" and exits 0, or the failed condition and exits 1.
#include "launch_plan.h"

#include <cstdlib>
#include <random>

static long g_checks = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    ++g_checks;                                                      \
    if (!(c)) {                                                      \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);            \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static std::mt19937_64 g_rng(0x57a61e5);
static int64_t rnd(int64_t lo, int64_t hi) { return lo + (int64_t)(g_rng() % (uint64_t)(hi - lo + 1)); }  // inclusive
template <typename T>
static T pick(std::initializer_list<T> l) { return l.begin()[rnd(0, (int64_t)l.size() - 1)]; }

// ---- the table block ---------------------------------------------------------------------------------------------------------------
struct raw_table {
  std::vector<uint8_t> bytes;
  size_t elem, count;
};
static void add_as(ww_table_block &tb, ww_bump &ref, const raw_table &t, size_t &off_tb, size_t &off_ref) {
  const void *p = t.count ? t.bytes.data() : nullptr;
  switch (t.elem) {
    case 1: off_tb = tb.add((const uint8_t *)p, t.count); off_ref = (size_t)((char *)ref.take<uint8_t>(t.count) - ref.base); break;
    case 4: off_tb = tb.add((const int32_t *)p, t.count); off_ref = (size_t)((char *)ref.take<int32_t>(t.count) - ref.base); break;
    case 8: off_tb = tb.add((const int64_t *)p, t.count); off_ref = (size_t)((char *)ref.take<int64_t>(t.count) - ref.base); break;
    case sizeof(wv_seg): off_tb = tb.add((const wv_seg *)p, t.count); off_ref = (size_t)((char *)ref.take<wv_seg>(t.count) - ref.base); break;
    default: off_tb = tb.add((const rs_tile *)p, t.count); off_ref = (size_t)((char *)ref.take<rs_tile>(t.count) - ref.base); break;
  }
}
static void check_tables() {
  static_assert(sizeof(wv_seg) == 16 && sizeof(rs_tile) == 72 && sizeof(rows_tile) == 32 && sizeof(feed_str) == 40 && sizeof(feed_grp) == 16 &&
                    sizeof(wv_feed_seg) == 24 && sizeof(wv_feed_pool) == 24,
                "the kernels read these layouts");
  for (int it = 0; it < 400; ++it) {
    const int n = (int)rnd(0, 6);
    std::vector<raw_table> tabs((size_t)n);
    size_t need = 0;
    for (int i = 0; i < n; ++i) {
      raw_table &t = tabs[i];
      t.elem = pick<size_t>({1, 4, 8, sizeof(wv_seg), sizeof(rs_tile)});
      t.count = (size_t)pick<int64_t>({0, 0, 1, 3, 16, 32, 64, 255, 256, 257, rnd(1, 700)});
      if (it % 5 == 1 && (i == 0 || i == n - 1)) t.count = 0;  // empty first / last
      t.bytes.resize(t.count * t.elem);
      for (uint8_t &b : t.bytes) b = (uint8_t)rnd(1, 255);  // (never 0: a gap cannot pass for data)
      need += ww_bump::need(t.count, t.elem);
    }
    ww_table_block tb;
    std::vector<char> arena(need + 1);
    ww_bump ref(arena.data(), need);
    std::vector<size_t> offs((size_t)n);
    for (int i = 0; i < n; ++i) {
      size_t a = 0, b = 0;
      const size_t before = tb.bytes();
      add_as(tb, ref, tabs[i], a, b);
      CHECK(a == b && a % 256 == 0);
      if (tabs[i].count == 0) CHECK(tb.bytes() == before);  // an empty table costs nothing
      offs[i] = a;
    }
    CHECK(tb.bytes() == need && tb.bytes() == ref.off);
    std::vector<uint8_t> block(tb.bytes(), 0xAB);  // exactly sized: a byte past it is a sanitizer report
    tb.pack(block.data());
    std::vector<uint8_t> want(tb.bytes(), 0);
    for (int i = 0; i < n; ++i)
      if (tabs[i].count) memcpy(want.data() + offs[i], tabs[i].bytes.data(), tabs[i].bytes.size());
    CHECK(block == want);  // the tables round-trip, and every other byte is zero
  }
  // join(): lists that a kernel indexes as one table lie back to back, and the block is that of the concatenation
  for (int it = 0; it < 200; ++it) {
    std::vector<int32_t> head((size_t)rnd(0, 40), 7);
    std::vector<rs_tile> a((size_t)pick<int64_t>({0, 1, 5, rnd(0, 60)})), b((size_t)pick<int64_t>({0, 2, rnd(0, 60)})), c((size_t)pick<int64_t>({0, 3}));
    std::vector<int64_t> tail((size_t)rnd(0, 9), -1);
    for (auto *v : {&a, &b, &c})
      for (rs_tile &t : *v) t.first = rnd(1, 1 << 30), t.n = (int32_t)rnd(1, 999);
    std::vector<rs_tile> all(a);
    all.insert(all.end(), b.begin(), b.end());
    all.insert(all.end(), c.begin(), c.end());
    ww_table_block j, w;
    const size_t jh = j.add(head), ja = j.add(a);
    j.join(b);
    j.join(c);
    const size_t jt = j.add(tail);
    const size_t wh = w.add(head), wa = w.add(all), wt = w.add(tail);
    CHECK(jh == wh && ja == wa && jt == wt && j.bytes() == w.bytes());
    std::vector<uint8_t> bj(j.bytes(), 0xAB), bw(w.bytes(), 0xCD);
    j.pack(bj.data());
    w.pack(bw.data());
    CHECK(bj == bw);
  }
}

// ---- the CRNN's sequences ----------------------------------------------------------------------------------------------------------
// the shipped geometry: a window of T = 151 rows, 19 time positions of a 20-row field at stride 8, 6 rows of zero padding in front
static const int C_T = 151, C_PT = 6, C_OT = 19, C_ST = 8;

static void check_crnn_case(const std::vector<int64_t> &row0, const std::vector<int32_t> &nws, int hop, int64_t mel_rows) {
  const int n_seg = (int)nws.size(), g = crnn_gcd8(hop);
  CHECK(hop % g == 0 && 8 % g == 0 && (g == 8 || (hop / g) % 2 == 1));  // g = gcd(hop, 8)
  crnn_seg_group gp;
  int64_t total = 0, done = 0;
  for (int32_t v : nws) total += v;
  for (int s0 = 0; s0 < n_seg; s0 = gp.next) {
    CHECK(crnn_plan_group(row0.data(), nws.data(), n_seg, hop, C_T, C_PT, C_OT, C_ST, mel_rows, s0, gp) == WW_OK);
    CHECK(gp.next > s0 && gp.next <= n_seg);
    int64_t nW = 0, nI = 0;
    int nonempty = 0;
    for (int s = s0; s < gp.next; ++s) {
      nW += nws[s];
      nonempty += nws[s] > 0;
      if (nws[s]) nI += ((int64_t)(nws[s] - 1) * hop + 128) / g + 1;  // fields at 0, g, 2 g .. up to the last window's position 17
    }
    CHECK(gp.nW == nW && gp.nI == nI && (int64_t)gp.i0.size() == nW);
    CHECK(nW <= WW_SEG_GROUP || nonempty == 1);
    if (gp.next < n_seg) CHECK(nW + nws[gp.next] > WW_SEG_GROUP);  // (the group was full: no sequence was left out for nothing)
    // what each output row of the three lists holds, from the tiles
    std::vector<int64_t> field[3] = {std::vector<int64_t>((size_t)nI), std::vector<int64_t>((size_t)nW), std::vector<int64_t>((size_t)nW)};
    std::vector<int> cover[3] = {std::vector<int>((size_t)nI, 0), std::vector<int>((size_t)nW, 0), std::vector<int>((size_t)nW, 0)};
    std::vector<int> seq_of[3];
    for (int s = s0; s < gp.next; ++s)
      if (nws[s]) {
        seq_of[0].insert(seq_of[0].end(), (size_t)(((int64_t)(nws[s] - 1) * hop + 128) / g + 1), s);
        seq_of[1].insert(seq_of[1].end(), (size_t)nws[s], s);
      }
    seq_of[2] = seq_of[1];
    int64_t next_int = 0;
    for (const rows_tile &t : gp.tiles) {
      CHECK(t.kind >= 0 && t.kind <= 2 && t.count >= 1 && t.count <= 16 && t.out_row >= 0);
      CHECK(t.out_row + t.count <= (int64_t)cover[t.kind].size());
      CHECK(t.stride == (t.kind == 0 ? g : hop));
      CHECK(seq_of[t.kind][(size_t)t.out_row] == seq_of[t.kind][(size_t)(t.out_row + t.count - 1)]);  // no tile spans two sequences
      if (t.kind == 0) {
        CHECK(t.out_row == next_int);  // the interior rows in order, without a gap
        next_int += t.count;
      }
      for (int p = 0; p < t.count; ++p) {
        ++cover[t.kind][(size_t)(t.out_row + p)];
        field[t.kind][(size_t)(t.out_row + p)] = t.start + (int64_t)p * t.stride;
      }
    }
    for (int k = 0; k < 3; ++k)
      for (int c : cover[k]) CHECK(c == 1);
    // the 19 fields gru_tail_kernel gathers for every window
    int64_t w = 0;
    for (int s = s0; s < gp.next; ++s)
      for (int k = 0; k < nws[s]; ++k, ++w)
        for (int t = 0; t < C_OT; ++t) {
          const int64_t want = row0[s] + (int64_t)k * hop + (int64_t)C_ST * t - C_PT;
          if (t == 0) CHECK(field[1][(size_t)w] == want);
          else if (t == C_OT - 1) CHECK(field[2][(size_t)w] == want);
          else {
            const int64_t i = gp.i0[(size_t)w] + (int64_t)(t - 1) * (8 / g);
            CHECK(i >= 0 && i < nI && seq_of[0][(size_t)i] == s && field[0][(size_t)i] == want);
          }
        }
    done += nW;
  }
  CHECK(done == total);  // the groups concatenated: every window once, in the call's order
}

static void check_crnn() {
  auto run = [](std::vector<int32_t> nws, int hop, bool odd_rows) {
    std::vector<int64_t> row0;
    int64_t mel_rows = C_T;
    for (int32_t nw : nws) {
      row0.push_back(odd_rows ? 2 * rnd(0, 400) + 1 : rnd(0, 800));
      if (nw) mel_rows = std::max(mel_rows, row0.back() + (int64_t)(nw - 1) * hop + C_T);  // the last window just fits
    }
    check_crnn_case(row0, nws, hop, mel_rows);
  };
  for (int hop = 1; hop <= 8; ++hop) {
    run({}, hop, false);
    run({0}, hop, false);
    run({40, 0, 1, 15, 16, 17, 333, 2}, hop, true);
    run({1}, hop, true);
    run({0, 0, 5000, 0}, hop, true);
  }
  run({WW_SEG_GROUP + 7232}, 2, true);                // one sequence larger than a group
  run({3, WW_SEG_GROUP + 1, 0, 4}, 3, false);
  run({20000, 12768, 1}, 2, false);                   // sums that meet and straddle the limit
  run({20000, 12769, 1}, 1, true);
  run({16385, 16385, 16385}, 2, false);
  run({WW_SEG_GROUP, 0, 1, WW_SEG_GROUP - 1, 1, 1}, 8, true);
  for (int it = 0; it < 300; ++it) {
    std::vector<int32_t> nws((size_t)rnd(0, 8));
    for (int32_t &nw : nws) nw = (int32_t)pick<int64_t>({0, 1, 15, 16, 17, rnd(1, 40), rnd(1, 3000)});
    run(nws, (int)rnd(1, 8), it % 2 == 0);
  }
  // the two refusals, with the texts the library has always given
  crnn_seg_group gp;
  const int64_t r0[3] = {0, 10, 5};
  const int32_t neg[3] = {4, -1, 2}, fit[3] = {4, 5, 2};
  CHECK(crnn_plan_group(r0, neg, 3, 2, C_T, C_PT, C_OT, C_ST, 1000, 0, gp) == WW_EINVAL && !strcmp(gp.err, "negative window count in sequence 1"));
  CHECK(crnn_plan_group(r0, fit, 3, 2, C_T, C_PT, C_OT, C_ST, 10 + 4 * 2 + C_T, 0, gp) == WW_OK);
  CHECK(crnn_plan_group(r0, fit, 3, 2, C_T, C_PT, C_OT, C_ST, 10 + 4 * 2 + C_T - 1, 0, gp) == WW_EINVAL &&
        !strcmp(gp.err, "sequence 1: windows leave the mel buffer"));
  const int64_t rneg[1] = {-1};
  CHECK(crnn_plan_group(rneg, fit, 1, 2, C_T, C_PT, C_OT, C_ST, 1000, 0, gp) == WW_EINVAL && !strcmp(gp.err, "sequence 0: windows leave the mel buffer"));
}

// ---- a segments call's descriptors: the whole-call walk and the explicit row list -------------------------------------------------
static void check_seg_walk() {
  const int hop = 2;
  const int64_t r0[3] = {7, 1000, 400};
  const int32_t nw[3] = {3, 0, 2};
  const int64_t mel_rows = 400 + (2 - 1) * hop + C_T;  // sequence 2's last window ends on the buffer's last row
  char err[WW_SEG_ERR];
  int64_t W = -1;
  CHECK(seg_walk(r0, nw, 3, hop, C_T, mel_rows, &W, err) == WW_OK && W == 5);  // (an empty sequence's row0 is never looked at)
  std::vector<int64_t> rows(1, -5), want(1, -5);  // appended: what the list held stays
  for (int s = 0; s < 3; ++s)
    for (int k = 0; k < nw[s]; ++k) want.push_back(r0[s] + (int64_t)k * hop);
  seg_rows(r0, nw, 3, hop, rows);
  CHECK(rows == want && (int64_t)rows.size() == 1 + W);
  // every fault: the walk's status and text, and crnn_plan_group's for the same call
  crnn_seg_group gp;
  auto refused = [&](const int64_t *row0, const int32_t *cnt, int64_t rows_in_buffer, const char *text) {
    memset(err, 0x55, sizeof err);
    CHECK(seg_walk(row0, cnt, 3, hop, C_T, rows_in_buffer, &W, err) == WW_EINVAL && !strcmp(err, text));
    CHECK(crnn_plan_group(row0, cnt, 3, hop, C_T, C_PT, C_OT, C_ST, rows_in_buffer, 0, gp) == WW_EINVAL && !strcmp(gp.err, text));
  };
  const int32_t neg[3] = {3, -1, 2};
  refused(r0, neg, mel_rows, "negative window count in sequence 1");
  refused(r0, nw, mel_rows - 1, "sequence 2: windows leave the mel buffer");  // its last window one row past the buffer
  const int64_t rneg[3] = {-1, 1000, 400};
  refused(rneg, nw, mel_rows, "sequence 0: windows leave the mel buffer");
  // no sequence: no window, no pointer read, nothing appended
  W = -1;
  rows.clear();
  CHECK(seg_walk(nullptr, nullptr, 0, hop, C_T, 0, &W, err) == WW_OK && W == 0);
  seg_rows(nullptr, nullptr, 0, hop, rows);
  CHECK(rows.empty());
}

// ---- the Wavenet's cuts ------------------------------------------------------------------------------------------------------------
static void check_wave() {
  for (int it = 0; it < 400; ++it) {
    const int rf = pick<int>({1, 2, 45, 181, 367}), n_seq = (int)rnd(0, 6), n_out = (int)rnd(1, 3);
    const int64_t seg_opt = it % 2 ? 0 : pick<int64_t>({1, 7, 192, rnd(1, 600)});  // the library's choice, or an explicit length
    std::vector<int64_t> offs(1, rnd(0, 50));
    for (int s = 0; s < n_seq; ++s) {
      int64_t len = pick<int64_t>({0, 1, 191, 192, 193, rnd(1, 5000), rnd(1, 5000)});
      if (it % 50 == 7 && seg_opt == 0) len = rnd(100000, 400000);
      if (seg_opt > 0 && seg_opt < 8) len = std::min<int64_t>(len, 300);
      offs.push_back(offs.back() + len);
    }
    const int64_t total_rows = offs.back() + rnd(0, 9);
    wave_seq_plan pl;
    wave_seq_make_plan(rf, n_out, seg_opt, total_rows, offs.data(), n_seq, 1, WAVE_SEQ_IDS_NONE, it % 3 == 0, it % 4 == 0, pl);
    size_t at = 0;
    int64_t max_len = 0;
    for (int s = 0; s < n_seq; ++s) {
      const int64_t o = offs[s], len = offs[s + 1] - o;
      max_len = std::max(max_len, len);
      for (int64_t done = 0; done < len;) {
        CHECK(at < pl.segs.size());
        const wv_seg &sg = pl.segs[at++];
        CHECK(sg.skip == std::min<int64_t>(done, rf - 1));  // the rows in front of it, as far as the receptive field reaches
        CHECK(sg.row0 >= o && sg.row0 + sg.skip == o + done);
        CHECK(sg.n > sg.skip && done + (sg.n - sg.skip) <= len);
        if (seg_opt > 0) CHECK(sg.n - sg.skip == std::min<int64_t>(seg_opt, len - done));
        done += sg.n - sg.skip;
      }
    }
    CHECK(at == pl.segs.size() && pl.max_len == max_len);
    CHECK(pl.b_segs == ww_bump::need(pl.segs.size(), sizeof(wv_seg)) && pl.b_offs == ww_bump::need((size_t)n_seq + 1, 8));
    CHECK(pl.b_z == (it % 3 == 0 ? ww_bump::need((size_t)total_rows * n_out, 4) : 0) && pl.b_pool == (it % 4 == 0 ? ww_bump::need((size_t)total_rows * n_out, 4) : 0));
  }
}

// ---- the feed ----------------------------------------------------------------------------------------------------------------------
static void check_feed() {
  const int hop = 160;
  for (int it = 0; it < 400; ++it) {
    const int S = (int)rnd(1, 9), T = pick<int>({8, 29, 182}), rf = pick<int>({45, 181});
    const int64_t seg_opt = it % 2 ? 0 : pick<int64_t>({1, 100, 192, rnd(1, 700)});
    std::vector<int> fill((size_t)S), pos((size_t)S), order((size_t)S);
    for (int s = 0; s < S; ++s) fill[s] = (int)rnd(0, 511), pos[s] = (int)rnd(0, T), order[s] = s;
    std::shuffle(order.begin(), order.end(), g_rng);
    const int n = (int)rnd(0, S);
    std::vector<int32_t> ids(order.begin(), order.begin() + n);
    std::vector<int64_t> so(1, rnd(0, 99)), ro(1, 0);
    for (int i = 0; i < n; ++i) {
      const int64_t k = pick<int64_t>({0, 1, 159, 160, 161, 511, 512, 513, rnd(0, 3000), rnd(0, 3000), rnd(3000, 60000)});
      const int64_t tot = fill[ids[i]] + k, r = tot >= 512 ? (tot - 512) / hop + 1 : 0;  // the framing rule (feed_check)
      so.push_back(so.back() + k);
      ro.push_back(ro.back() + r);
    }
    feed_plan pl;
    feed_make_plan(ids.data(), n, so.data(), ro.data(), fill.data(), pos.data(), T, rf, seg_opt, pl);
    CHECK((int)pl.str.size() == n);
    size_t ag = 0, as = 0, al = 0, ap = 0, ar = 0;
    for (int i = 0; i < n; ++i) {
      const int s = ids[i];
      const int64_t k = so[i + 1] - so[i], r = ro[i + 1] - ro[i];
      const feed_str &d = pl.str[i];
      CHECK(d.s_off == so[i] - so[0] && d.k == k && d.r_off == ro[i] && d.sid == s && d.fill == fill[s] && d.rows == r && d.pos == pos[s]);
      if (k == 0) continue;  // an empty packet gets nothing
      if (r == 0) {  // samples but no new row: the one state-only group
        CHECK(ag < pl.grp.size() && pl.grp[ag].i == i && pl.grp[ag].f0 == 0 && pl.grp[ag].nf == 0);
        ++ag;
        continue;
      }
      for (int64_t f = 0; f < r;) {
        CHECK(ag < pl.grp.size());
        const feed_grp &gq = pl.grp[ag++];
        CHECK(gq.i == i && gq.f0 == f && gq.nf >= 1 && gq.nf <= FEED_GROUP && f + gq.nf <= r);
        f += gq.nf;
      }
      if (r <= 16 && r <= T) {
        CHECK(as < pl.small.size());
        const wv_feed_seg &sg = pl.small[as++];
        CHECK(sg.row0 == ro[i] && sg.n == r && sg.skip == 0 && sg.sid == s && sg.flags == 3);
        continue;
      }
      const size_t first = al;
      for (int64_t done = 0; done < r;) {
        CHECK(al < pl.large.size());
        const wv_feed_seg &sg = pl.large[al++];
        const int64_t kept = sg.n - sg.skip;
        CHECK(sg.sid == s && kept > 0 && done + kept <= r);
        CHECK(sg.skip == (done ? rf - 1 : 0) && (sg.flags & 1) == (done ? 0 : 1));
        CHECK(sg.row0 >= ro[i] && sg.row0 + sg.skip == ro[i] + done);  // the warm-up lies inside the call's rows
        done += kept;
        CHECK(((sg.flags & 2) != 0) == (done == r) && (sg.flags & ~3) == 0);
        if (done == r) CHECK(kept >= WV_FEED_HIST_ROWS || al - first == 1);
      }
      for (int64_t k0 = 0; k0 < r; k0 += WW_FEED_POOL_ROWS) {  // a pool tile covers rows [k0, k0 + WW_FEED_POOL_ROWS) of the stream's r
        CHECK(ap < pl.pool.size());
        const wv_feed_pool &p = pl.pool[ap++];
        CHECK(p.row0 == ro[i] && p.n == r && p.sid == s && p.k0 == k0);
      }
      CHECK(ar < pl.ringt.size() && pl.ringt[ar].row0 == ro[i] && pl.ringt[ar].n == r && pl.ringt[ar].sid == s);
      ++ar;
    }
    CHECK(ag == pl.grp.size() && as == pl.small.size() && al == pl.large.size() && ap == pl.pool.size() && ar == pl.ringt.size());
  }
}

// ---- the resampler -----------------------------------------------------------------------------------------------------------------
// y[m] = sum over k of h[m * down - k * up] x[k], |m * down - k * up| <= half (resample.hip).  The geometry as ww_resampler_create
// derives it from the two rates (default filter: 32 zero crossings, roll-off 0.945; 256 threads per tile, up == 1 table padded to 4).
static int64_t gcd64(int64_t a, int64_t b) { return b ? gcd64(b, a % b) : a; }
static int64_t floor_div(int64_t a, int64_t b) { return a / b - (a % b != 0 && ((a < 0) != (b < 0))); }
static rs_geom make_geom(int rate_in, int rate_out) {
  rs_geom r;
  const int64_t g = gcd64(rate_in, rate_out), up = r.up = rate_out / g, down = r.down = rate_in / g;
  if (up == 1 && down == 1) {
    r.identity = true;
    return r;
  }
  const double f2 = 0.945 * (double)std::min(rate_in, rate_out) / (double)((int64_t)rate_in * up);
  r.half = (int64_t)__builtin_ceil(32.0 / f2);
  r.tpp = (2 * r.half + 1 + up - 1) / up;
  for (int64_t ne = 256; ne >= 64 && !r.ne8; ne /= 2)
    if (rs_phase_span(&r, RS_R, ne) <= RS_XCAP) r.ne8 = (int32_t)ne;
  for (int64_t ne = 256; ne >= 1 && !r.ne1; ne /= 2)
    if (rs_phase_span(&r, 1, ne) <= RS_XCAP) r.ne1 = (int32_t)ne;
  if (up == 1) {
    const int64_t n_u = (RS_R1 - 1) * down + 2 * r.half + 1, n_u_pad = (n_u + 3) / 4 * 4;
    const int64_t lanes = std::min<int64_t>(256, (RS_XCAP - n_u_pad) / (RS_R1 * down) + 1);
    if (n_u_pad <= RS_XCAP && lanes >= 1) r.n_u = (int32_t)n_u_pad, r.lanes1 = (int32_t)lanes;
  }
  return r;
}

// The class of a pair of the twelve standard rates as the planner's arithmetic gives it for the default filter, worked out by hand
// once and written down: {up == 1 form?, ne8, ne1, lanes1}.  A change of RS_XCAP, RS_R, RS_R1 or of the span formulas that moves a
// pair into another class shows here, and with it which GPU test no longer reaches the class it was chosen for.
struct rs_class {
  bool decim;
  int32_t ne8, ne1, lanes1;
};
static rs_class want_class(int rate_in, int rate_out) {
  struct row {
    int in, out;
    rs_class c;
  };
  static const row rows[] = {
      {192000, 8000, {true, 0, 256, 63}},      {176400, 11025, {true, 64, 256, 100}},   {96000, 8000, {true, 64, 256, 136}},
      {192000, 16000, {true, 64, 256, 136}},   {88200, 11025, {true, 128, 256, 209}},   {176400, 22050, {true, 128, 256, 209}},
      {192000, 24000, {true, 128, 256, 209}},  {48000, 8000, {true, 128, 256, 256}},    {96000, 16000, {true, 128, 256, 256}},
      {192000, 32000, {true, 128, 256, 256}},  {32000, 11025, {false, 0, 256, 0}},      {96000, 11025, {false, 0, 256, 0}},
      {176400, 8000, {false, 0, 256, 0}},      {192000, 11025, {false, 0, 256, 0}},     {192000, 22050, {false, 0, 256, 0}},
      {88200, 8000, {false, 64, 256, 0}},      {176400, 16000, {false, 64, 256, 0}},    {44100, 8000, {false, 128, 256, 0}},
      {48000, 11025, {false, 128, 256, 0}},    {88200, 16000, {false, 128, 256, 0}},    {96000, 22050, {false, 128, 256, 0}},
      {176400, 24000, {false, 128, 256, 0}},   {176400, 32000, {false, 128, 256, 0}},   {192000, 44100, {false, 128, 256, 0}},
      {500000, 16000, {false, 0, 256, 0}}};  // (the last: not a standard rate - the longest chain a stream bank takes, tpp = 2117)
  for (const row &w : rows)
    if (w.in == rate_in && w.out == rate_out) return w.c;
  const int64_t g = gcd64(rate_in, rate_out);
  if (rate_out / g == 1) return {true, 256, 256, 256};  // the 18 pairs with down in {2, 3, 4}
  return {false, 256, 256, 0};                          // the remaining 90, and 16050 / 8050 -> 16000 (up = 320)
}

static void check_resample() {
  static const int standard[] = {8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000};
  std::vector<std::pair<int, int>> pairs;
  for (int a : standard)
    for (int b : standard)
      if (a != b) pairs.push_back({a, b});
  CHECK(pairs.size() == 132);
  for (int rate : {16000, 500000, 16050, 8050}) pairs.push_back({rate, 16000});
  int n_decim18 = 0, n_phase90 = 0;
  for (size_t pi = 0; pi < pairs.size(); ++pi) {
    const int rate = pairs[pi].first, rate_out = pairs[pi].second;
    const rs_geom r = make_geom(rate, rate_out);
    CHECK(r.identity == (rate == rate_out));
    if (!r.identity) CHECK(r.ne1 >= 1 && 2 * r.down + r.tpp + 2 <= RS_XCAP);
    if (!r.identity) {
      const rs_class w = want_class(rate, rate_out);
      CHECK((r.up == 1 && r.lanes1 > 0) == w.decim && r.ne8 == w.ne8 && r.ne1 == w.ne1 && r.lanes1 == w.lanes1);
      if (pi < 132) {  // (the two classes the table names by their size only)
        n_decim18 += w.decim && w.ne8 == 256;
        n_phase90 += !w.decim && w.ne8 == 256;
      }
    }
    std::vector<int64_t> q_of_phase((size_t)r.up);  // m mod up of the outputs of phase p = m * down mod up
    for (int64_t q = 0; q < r.up; ++q) q_of_phase[(size_t)((q * r.down) % r.up)] = q;
    const int64_t a_tile = r.identity ? RS_COPY : r.up == 1 && r.lanes1 ? (int64_t)r.lanes1 * RS_R1 : r.ne8 ? (int64_t)r.ne8 / r.up * RS_R + 1 : 64;
    // The walk below costs about (outputs x tiles) per segment, and a segment of 2 * RS_R * up outputs is large where up is: fewer
    // iterations for such a pair, never fewer than six.  The first two iterations take fixed counts (without and with in_first /
    // out_first), so that the threshold between the two phase forms and the tile's edge are walked for every pair however few the
    // random iterations are.
    const int iters = (int)std::max<int64_t>(6, std::min<int64_t>(40, 400000 / (2 * RS_R * r.up + 3 * a_tile)));
    const int64_t fixed[2][4] = {{2 * RS_R * r.up - 1, a_tile, 1, 0}, {2 * RS_R * r.up, a_tile + 1, 2, 3 * a_tile + 9}};
    for (int it = 0; it < iters; ++it) {
      const int n_seg = it < 2 ? 4 : (int)rnd(1, 4);
      std::vector<int64_t> so(1, rnd(0, 77)), oo(1, rnd(0, 55)), in_first, out_first;
      for (int u = 0; u < n_seg; ++u) {
        const int64_t cnt = it < 2 ? fixed[it][u] : pick<int64_t>({0, 1, 2, rnd(1, 40), 2 * RS_R * r.up - 1, 2 * RS_R * r.up, rnd(1, a_tile), a_tile, a_tile + 1, rnd(1, 3 * a_tile + 9)});
        oo.push_back(oo.back() + cnt);
        so.push_back(so.back() + rnd(0, 5000));
        in_first.push_back(it % 3 ? rnd(0, 1 << 20) : 0);
        out_first.push_back(it % 3 ? pick<int64_t>({0, 1, rnd(0, 100000), (int64_t)1 << 33}) : 0);
      }
      rs_plan pl;
      CHECK(rs_make_plan(&r, so.data(), it % 3 ? in_first.data() : nullptr, it % 3 ? out_first.data() : nullptr, oo.data(), n_seg, pl) == WW_OK);
      size_t used = 0;
      for (int u = 0; u < n_seg; ++u) {
        const int64_t cnt = oo[u + 1] - oo[u], m0 = out_first[u], m1 = m0 + cnt;
        if (cnt == 0) continue;  // (oo ascends strictly over the others: out_off names the segment)
        auto mine = [&](const std::vector<rs_tile> &v) {
          std::vector<rs_tile> t;
          for (const rs_tile &x : v)
            if (x.out_off == oo[u]) t.push_back(x);
          for (const rs_tile &x : t) {
            CHECK(x.in_off == so[u] && x.in_first == in_first[u] && x.n_in == so[u + 1] - so[u] && x.out_first == m0 && x.out_end == m1);
            CHECK(x.n >= 1 && x.n <= (r.identity ? RS_COPY : 256));
            if (!r.identity) CHECK(x.n_x >= 1 && x.n_x <= RS_XCAP);
          }
          used += t.size();
          return t;
        };
        const std::vector<rs_tile> cp = mine(pl.copy), dc = mine(pl.decim), p8 = mine(pl.ph8), p1 = mine(pl.ph1);
        const int form = r.identity ? 0 : r.up == 1 && r.lanes1 > 0 ? 1 : r.ne8 > 0 && cnt >= 2 * RS_R * r.up ? 2 : 3;
        CHECK(cp.empty() == (form != 0) && dc.empty() == (form != 1) && p8.empty() == (form != 2) && p1.empty() == (form != 3));
        const std::vector<rs_tile> &tl = form == 0 ? cp : form == 1 ? dc : form == 2 ? p8 : p1;
        const int R = form == 2 ? RS_R : 1;
        if (form >= 2)  // what resample_phase_kernel's items read of the staged span (padded taps included): all of it staged
          for (const rs_tile &t : tl)
            for (int64_t e = t.first; e < t.first + t.n; ++e) {
              const int64_t A = e / r.up, ph = e % r.up, cq = q_of_phase[(size_t)ph] * r.down / r.up, jmax = (r.half - ph) / r.up;
              const int64_t lo = A * R * r.down + cq - jmax - t.k_lo;
              CHECK(lo >= 0 && lo + (int64_t)(R - 1) * r.down + r.tpp - 1 < t.n_x);
            }
        for (int64_t m = m0; m < m1; ++m) {
          // the taps of output m reach inputs k_min .. k_max
          const int64_t k_min = r.identity ? m : -floor_div(-(m * r.down - r.half), r.up), k_max = r.identity ? m : floor_div(m * r.down + r.half, r.up);
          int owners = 0;
          for (const rs_tile &t : tl) {
            bool in = false;
            if (form == 0) {
              in = m >= t.first && m < t.first + t.n;
            } else if (form == 1) {  // lane l of t.n owns outputs t.first + l * RS_R1 + (0 .. RS_R1 - 1)
              in = m >= t.first && m < t.first + (int64_t)t.n * RS_R1;
              if (in) CHECK(t.k_lo == t.first * r.down - r.half && (int64_t)(t.n - 1) * RS_R1 * r.down + r.n_u <= t.n_x);  // (what the lanes read)
            } else {  // item e = A * up + p owns outputs (A * R + j) * up + q, j < R, of phase p = m * down mod up
              const int64_t A = (m / r.up) / R, e = A * r.up + (m * r.down) % r.up;
              in = e >= t.first && e < t.first + t.n;
            }
            if (!in) continue;
            ++owners;
            if (form) CHECK(t.k_lo <= k_min && k_max < t.k_lo + t.n_x);
          }
          CHECK(owners == 1);
        }
      }
      CHECK(used == pl.count());
    }
  }
  CHECK(n_decim18 == 18 && n_phase90 == 90);
}

int main() {
  check_tables();
  check_crnn();
  check_seg_walk();
  check_wave();
  check_feed();
  check_resample();
  printf("ok %ld\n", g_checks);
  return 0;
}
