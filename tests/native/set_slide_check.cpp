// set_slide_check - the host half of a model set's sliding form on the CPU, under Address + UB sanitizer
// (tests/test_set_slide_host.py): csrc/launch_plan.h's crnn_plan_group with the window cap as a parameter, and csrc/model_set.h's
// check of the member list a call brings.  Prints "ok <checks>" and exits 0, or the failed condition and exits 1.
//
// A set's call of n_members slots keeps n_members x windows of a group at or below WW_SEG_GROUP by planning with the cap
// WW_SEG_GROUP / n_members.  The tile table and i0 of a group are shared by every slot, so they must be what the single-model plan
// holds for the same sequences: the cap may only move where the groups are cut.
#include "launch_plan.h"
#include "model_set.h"

#include <cstdlib>

static long g_checks = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    ++g_checks;                                                      \
    if (!(c)) {                                                      \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);            \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static const int C_T = 151, C_PT = 6, C_OT = 19, C_ST = 8;  // the shipped geometry (launch_plan_check.cpp)

struct flat_plan {
  std::vector<rows_tile> tiles;  // out_row in the CALL's rows of its list (group bases added)
  std::vector<int64_t> i0;       // in the call's interior rows
  int64_t nI = 0, nW = 0;
  int groups = 0;
};

// every group of the call planned with window cap `cap`, concatenated; `budget` / `n_members`: what the groups must respect
static flat_plan plan_all(const std::vector<int64_t> &row0, const std::vector<int32_t> &nws, int hop, int64_t mel_rows, int64_t cap, int n_members,
                          int64_t budget) {
  const int n_seg = (int)nws.size();
  flat_plan f;
  crnn_seg_group gp;
  for (int s0 = 0; s0 < n_seg; s0 = gp.next) {
    CHECK(crnn_plan_group(row0.data(), nws.data(), n_seg, hop, C_T, C_PT, C_OT, C_ST, mel_rows, s0, gp, cap) == WW_OK);
    CHECK(gp.next > s0 && gp.next <= n_seg);  // whole sequences [s0, next): no group splits one
    int64_t nW = 0;
    int nonempty = 0;
    for (int s = s0; s < gp.next; ++s) {
      nW += nws[s];
      nonempty += nws[s] > 0;
    }
    CHECK(gp.nW == nW && (int64_t)gp.i0.size() == nW);
    CHECK((int64_t)n_members * nW <= budget || nonempty == 1);
    if (gp.next < n_seg) CHECK(nW + nws[gp.next] > cap);  // the group was full
    for (rows_tile t : gp.tiles) {
      CHECK(t.kind >= 0 && t.kind <= 2 && t.count >= 1 && t.count <= 16);
      CHECK(t.out_row >= 0 && t.out_row + t.count <= (t.kind == 0 ? gp.nI : gp.nW));  // inside the group's plane of its list
      t.out_row += t.kind == 0 ? f.nI : f.nW;
      f.tiles.push_back(t);
    }
    for (int64_t i : gp.i0) {
      CHECK(i >= 0 && i + (int64_t)(C_OT - 3) * (8 / crnn_gcd8(hop)) < gp.nI);  // positions 1..17 inside the group's interior plane
      f.i0.push_back(i + f.nI);
    }
    f.nI += gp.nI;
    f.nW += gp.nW;
    ++f.groups;
  }
  return f;
}

static bool same_tile(const rows_tile &a, const rows_tile &b) {
  return a.start == b.start && a.out_row == b.out_row && a.stride == b.stride && a.count == b.count && a.kind == b.kind;
}

static void check_case(const std::vector<int32_t> &nws, int hop, int64_t first_row) {
  std::vector<int64_t> row0;
  int64_t at = first_row, total = 0;
  for (size_t s = 0; s < nws.size(); ++s) {
    row0.push_back(at);
    at += (nws[s] ? (int64_t)(nws[s] - 1) * hop + C_T : 0) + 5 + (int64_t)(7 * s) % 26;  // 5..30 rows of other data between sequences
    total += nws[s];
  }
  const int64_t mel_rows = at;
  const flat_plan ref = plan_all(row0, nws, hop, mel_rows, WW_SEG_GROUP, 1, WW_SEG_GROUP);
  CHECK(ref.nW == total && (int64_t)ref.i0.size() == total);
  // every interior field, left edge and right edge of the call has exactly one owner tile
  auto one_owner = [&](const flat_plan &f) {
    std::vector<int> cover[3] = {std::vector<int>((size_t)f.nI, 0), std::vector<int>((size_t)f.nW, 0), std::vector<int>((size_t)f.nW, 0)};
    for (const rows_tile &t : f.tiles)
      for (int p = 0; p < t.count; ++p) {
        CHECK(t.out_row + p < (int64_t)cover[t.kind].size());
        ++cover[t.kind][(size_t)(t.out_row + p)];
      }
    for (int k = 0; k < 3; ++k)
      for (int c : cover[k]) CHECK(c == 1);
  };
  one_owner(ref);
  for (int64_t budget : {(int64_t)40, (int64_t)48, (int64_t)WW_SEG_GROUP})
    for (int n_members : {1, 2, 3}) {
      const int64_t cap = std::max<int64_t>(budget / n_members, 1);  // ww_k_crnn_segments_forward's for a set's call
      const flat_plan f = plan_all(row0, nws, hop, mel_rows, cap, n_members, budget);
      CHECK(f.nI == ref.nI && f.nW == ref.nW && f.tiles.size() == ref.tiles.size() && f.i0 == ref.i0);
      for (size_t i = 0; i < f.tiles.size(); ++i) CHECK(same_tile(f.tiles[i], ref.tiles[i]));
      one_owner(f);
      if (budget == 40 && n_members == 3 && total > 13) CHECK(f.groups > ref.groups);  // (the cap did cut)
    }
}

static void check_plans() {
  for (int hop : {1, 2, 3, 8}) {
    check_case({0, 1, 16, 17, 40}, hop, 7);
    check_case({17, 0, 41, 1, 16}, hop, 0);       // 41: a sequence larger than the caps 40 and 48 / 2
    check_case({49, 1, 16, 17, 0, 100, 0}, hop, 3);
    check_case({1}, hop, 0);
    check_case({0, 0}, hop, 0);
    check_case({}, hop, 0);
  }
  check_case({5, WW_SEG_GROUP + 17, 0, 16, 17}, 2, 1);  // larger than the default cap too
  check_case({11000, 11000, 11000}, 8, 0);              // a third of the default budget each: three members cut after every sequence
  // the cap does not soften a refusal
  crnn_seg_group gp;
  const int64_t r0[2] = {0, 10};
  const int32_t neg[2] = {4, -1}, fit[2] = {4, 5};
  CHECK(crnn_plan_group(r0, neg, 2, 2, C_T, C_PT, C_OT, C_ST, 1000, 0, gp, 4) == WW_EINVAL && !strcmp(gp.err, "negative window count in sequence 1"));
  CHECK(crnn_plan_group(r0, neg, 2, 2, C_T, C_PT, C_OT, C_ST, 1000, 1, gp, 4) == WW_EINVAL && !strcmp(gp.err, "negative window count in sequence 1"));
  CHECK(crnn_plan_group(r0, fit, 2, 2, C_T, C_PT, C_OT, C_ST, 1000, 0, gp, 4) == WW_OK && gp.next == 1 && gp.nW == 4);  // (4 + 5 > 4: cut)
  CHECK(crnn_plan_group(r0, fit, 2, 2, C_T, C_PT, C_OT, C_ST, 10 + 4 * 2 + C_T - 1, 1, gp, 1) == WW_EINVAL &&
        !strcmp(gp.err, "sequence 1: windows leave the mel buffer"));
}

// the member list of ww_set_forward_segments_dev / ww_set_slide_forward (ww_set_check_ids, what = "members")
static void check_members() {
  char err[160];
  const int K = 3;
  strcpy(err, "untouched");
  CHECK(ww_set_check_ids(nullptr, 0, K, "members", err, sizeof err) == WW_OK);   // NULL: every member in order
  CHECK(ww_set_check_ids(nullptr, 5, K, "members", err, sizeof err) == WW_OK);
  const int32_t all[3] = {0, 1, 2}, dup[4] = {1, 1, 2, 1}, perm[2] = {2, 0};
  CHECK(ww_set_check_ids(all, 3, K, "members", err, sizeof err) == WW_OK);
  CHECK(ww_set_check_ids(dup, 4, K, "members", err, sizeof err) == WW_OK);       // duplicates are slots of their own
  CHECK(ww_set_check_ids(perm, 2, K, "members", err, sizeof err) == WW_OK);
  CHECK(ww_set_check_ids(all, 0, K, "members", err, sizeof err) == WW_OK);       // n_members = 0
  CHECK(!strcmp(err, "untouched"));
  const int32_t neg[3] = {0, 2, -1}, big[3] = {0, K, 1};
  CHECK(ww_set_check_ids(neg, 3, K, "members", err, sizeof err) == WW_EINVAL && strstr(err, "members[2] = -1"));
  CHECK(ww_set_check_ids(big, 3, K, "members", err, sizeof err) == WW_EINVAL && strstr(err, "members[1] = 3") && strstr(err, "0..2"));
  CHECK(ww_set_check_ids(neg, 2, K, "members", err, sizeof err) == WW_OK);       // (the bad entry lies behind the list's end)
}

int main() {
  check_plans();
  check_members();
  printf("ok %ld\n", g_checks);
  return 0;
}
