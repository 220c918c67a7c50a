// set_wave_seq_check - the host half of the Wavenet's sequence form over a model set on the CPU, under Address + UB sanitizer
// (tests/test_set_sequence_host.py): csrc/launch_plan.h's wave_seq_make_plan in its three id forms over random offset lists and slot lists, and
// csrc/model_set.h's check of the ids a call brings.  Prints "ok <checks>" and exits 0, or the failed condition and exits 1.
//
// A set's launch is segments x planes workgroups: workgroup (x, y) keeps rows [row0 + skip, row0 + n) of segment x and writes them
// into plane y.  In the by-sequence form (one plane) it finds its member through seg_seq[x], the sequence of segment x.
#include "launch_plan.h"
#include "model_set.h"

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

static std::mt19937_64 g_rng(0x5e7a11);
static int64_t rnd(int64_t lo, int64_t hi) { return lo + (int64_t)(g_rng() % (uint64_t)(hi - lo + 1)); }  // inclusive
template <typename T>
static T pick(std::initializer_list<T> l) { return l.begin()[rnd(0, (int64_t)l.size() - 1)]; }

static bool same_seg(const wv_seg &a, const wv_seg &b) { return a.row0 == b.row0 && a.n == b.n && a.skip == b.skip; }

static void check_case(int it) {
  const int rf = pick<int>({1, 2, 45, 181, 367}), n_seq = (int)rnd(0, 7), n_out = (int)rnd(1, 3);
  const int64_t seg_opt = it % 2 ? 0 : pick<int64_t>({1, 7, 192, 256, rnd(1, 600)});
  std::vector<int64_t> offs(1, rnd(0, 50));
  for (int s = 0; s < n_seq; ++s) {
    int64_t len = pick<int64_t>({0, 0, 1, 16, 181, 182, 191, 192, 193, 450, rnd(1, 5000)});
    if (seg_opt > 0 && seg_opt < 8) len = std::min<int64_t>(len, 300);
    offs.push_back(offs.back() + len);
  }
  const int64_t total_rows = offs.back() + rnd(0, 9);
  const bool need_z = it % 3 == 0, need_pool = it % 4 == 0;
  wave_seq_plan one;
  wave_seq_make_plan(rf, n_out, seg_opt, total_rows, offs.data(), n_seq, 1, WAVE_SEQ_IDS_NONE, need_z, need_pool, one);
  CHECK(one.b_ids == 0 && one.b_aux == 0 && one.seg_seq.empty());  // (no ids: the single model's plan)

  for (int form = 0; form < 2; ++form) {
    const bool by_seq = form == 1;
    const int planes = by_seq ? 1 : pick<int>({1, 1, 2, 3, 64, 65, 1024});  // (a slot list of that many ids, duplicates or not)
    wave_seq_plan pl;
    wave_seq_make_plan(rf, n_out, seg_opt, total_rows, offs.data(), n_seq, planes, by_seq ? WAVE_SEQ_IDS_BY_SEQ : WAVE_SEQ_IDS_BY_PLANE, need_z, need_pool, pl);
    // the cuts are the single model's, segment for segment: a member is weights, not geometry
    CHECK(pl.segs.size() == one.segs.size() && pl.max_len == one.max_len);
    for (size_t i = 0; i < pl.segs.size(); ++i) CHECK(same_seg(pl.segs[i], one.segs[i]));
    // what the plan reserved is what the tables take - segments, offsets, ids, the sequence of every segment - and planes x the
    // single model's scratch rows
    const size_t n_ids = by_seq ? (size_t)n_seq : (size_t)planes;
    CHECK(pl.b_segs == ww_bump::need(pl.segs.size(), sizeof(wv_seg)) && pl.b_offs == ww_bump::need((size_t)n_seq + 1, 8));
    CHECK(pl.b_ids == ww_bump::need(n_ids, 4));
    CHECK(pl.b_aux == (by_seq ? ww_bump::need(pl.segs.size(), 4) : 0));
    CHECK(pl.seg_seq.size() == (by_seq ? pl.segs.size() : 0));
    CHECK(pl.b_z == (need_z ? ww_bump::need((size_t)planes * total_rows * n_out, 4) : 0));
    CHECK(pl.b_pool == (need_pool ? ww_bump::need((size_t)planes * total_rows * n_out, 4) : 0));
    CHECK(pl.bytes() == pl.b_segs + pl.b_offs + pl.b_ids + pl.b_aux + pl.b_z + 2 * pl.b_pool);
    {
      std::vector<int32_t> ids(n_ids, 1);
      ww_table_block tb;
      tb.add(pl.segs);
      tb.add(offs.data(), (size_t)n_seq + 1);
      tb.add(ids.data(), n_ids);
      if (by_seq) tb.add(pl.seg_seq);
      CHECK(tb.bytes() == pl.b_segs + pl.b_offs + pl.b_ids + pl.b_aux);
    }
    // one plane of the slot form IS the single model's plan (which has no ids: its b_ids is the one difference)
    if (!by_seq && planes == 1) CHECK(pl.b_z == one.b_z && pl.b_pool == one.b_pool && pl.bytes() == one.bytes() + pl.b_ids && pl.seg_seq.empty());
    // every (sequence row, plane) has exactly one owner segment, which keeps it after a warm-up of min(s0, rf - 1) rows, and no
    // segment keeps a row outside every sequence
    const int shown = std::min(planes, 3);  // (the grid's second dimension repeats the segment list: three planes show it)
    std::vector<int> cover((size_t)shown * (size_t)total_rows, 0);
    for (int y = 0; y < shown; ++y)
      for (size_t x = 0; x < pl.segs.size(); ++x) {
        const wv_seg &sg = pl.segs[x];
        CHECK(sg.skip >= 0 && sg.n > sg.skip && sg.row0 >= 0 && sg.row0 + sg.n <= total_rows);
        for (int64_t r = sg.row0 + sg.skip; r < sg.row0 + sg.n; ++r) ++cover[(size_t)y * total_rows + r];
      }
    for (int y = 0; y < shown; ++y)
      for (int64_t r = 0; r < total_rows; ++r) CHECK(cover[(size_t)y * total_rows + r] == (r >= offs[0] && r < offs[n_seq] ? 1 : 0));
    size_t at = 0;
    for (int s = 0; s < n_seq; ++s) {
      const int64_t o = offs[s], len = offs[s + 1] - o;
      for (int64_t done = 0; done < len;) {
        CHECK(at < pl.segs.size());
        const wv_seg &sg = pl.segs[at];
        CHECK(sg.skip == std::min<int64_t>(done, rf - 1));  // the warm-up: the rows in front of it, as far as the receptive field reaches
        CHECK(sg.row0 + sg.skip == o + done && sg.row0 >= o && sg.row0 + sg.n <= o + len);  // (it reads its own sequence only)
        if (by_seq) CHECK(pl.seg_seq[at] == s);
        done += sg.n - sg.skip;
        ++at;
      }
    }
    CHECK(at == pl.segs.size());
  }
}

// the ids of ww_set_wave_sequence* (ww_set_check_ids: "seq_model" has n_seq entries, "members" n_members)
static void check_ids() {
  char err[160];
  const int K = 2;
  strcpy(err, "untouched");
  CHECK(ww_set_check_ids(nullptr, 7, K, "seq_model", err, sizeof err) == WW_OK);  // NULL: every sequence by member 0
  const int32_t route[7] = {0, 1, 1, 0, 1, 0, 0}, slots[3] = {1, 0, 1};
  CHECK(ww_set_check_ids(route, 7, K, "seq_model", err, sizeof err) == WW_OK);
  CHECK(ww_set_check_ids(slots, 3, K, "members", err, sizeof err) == WW_OK);
  CHECK(ww_set_check_ids(slots, 0, K, "members", err, sizeof err) == WW_OK);
  CHECK(!strcmp(err, "untouched"));
  const int32_t big[7] = {0, 1, 1, 0, 2, 0, 0}, neg[3] = {1, 0, -1};
  CHECK(ww_set_check_ids(big, 7, K, "seq_model", err, sizeof err) == WW_EINVAL && strstr(err, "seq_model[4] = 2") && strstr(err, "0..1"));
  CHECK(ww_set_check_ids(neg, 3, K, "members", err, sizeof err) == WW_EINVAL && strstr(err, "members[2] = -1"));
}

int main() {
  for (int it = 0; it < 600; ++it) check_case(it);
  check_ids();
  printf("ok %ld\n", g_checks);
  return 0;
}
