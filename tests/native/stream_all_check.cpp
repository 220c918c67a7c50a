// stream_all_check - csrc/stream_all.h (the host-only half of a stream bank's tick, and of the bank that runs every listed member of a
// model set on every stream) alone on the CPU, under Address + UB sanitizer (tests/test_stream_all_host.py compiles and runs it;
// nothing here touches a GPU).  Over K in {1, 3, 5} member slots, S in {1, 5} streams and the three launch forms, a script of 700
// ticks with every mix of the two flag bits (0 to 2 new rows per tick arise from the sample count by themselves) - several wraps of
// the mel ring (152 slots) and of the cache ring (144) - is held against a model written from the reference's loop
// (spokestack/wakeword/tflite.py:163-168: one frame whenever 512 samples are buffered, then the oldest 160 are dropped):
//   * the control words of every physical stream, the state parity of the one-launch form included;
//   * the descriptors of the three table-driven forms: `row` from the PHYSICAL stream, `aux` from the VIRTUAL one
//     (v * 144 + cache slot | v + emit * 65536), in (s, slot, k) order, and no more descriptors than the tables hold (2 S K);
//   * the tag slots to expect: 2 v + k, or the descriptor's index; each slot at most once, all inside [0, 2 S K);
//   * the post scatter [S][K][2]: entry (s, j, k) is what arrived in ITS slot, zeros beyond n_post[s];
//   * K = 1 gives v = s: an every-member bank of one slot plans what an ordinary bank plans;
//   * resets in the middle (mirrors zeroed as ww_stream_reset does) and the virtual ids of a reset;
//   * the member table [S K], and every refusal: of a creation (slots outside 1..64, full recompute, unknown flags, no streams,
//     S K > 65535 with 65535 itself allowed) and of a call on the wrong kind of bank, each with its reason;
//   * the id list of a reset or a move (sa_check_ids): no list, an empty one and 2 S ids pass; a negative count, more than 2 S ids and
//     an id out of range are refused, each alone with its reason, and in that order where two apply.
// Prints "ok <checks>" and exits 0; or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "stream_all.h"

static long n_checks = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    ++n_checks;                                                               \
    if (!(cond)) {                                                            \
      fprintf(stderr, "stream_all_check: %s (line %d)\n", #cond, __LINE__);  \
      exit(1);                                                                \
    }                                                                         \
  } while (0)

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)((rng_state >> 33) % n);
}

// the reference's loop for one tick of one stream: 320 samples arrive one by one
struct model_stream {
  int buffered = 0;      // samples in the window
  long rows = 0;         // mel rows written since the reset
  long posts = 0;        // posteriors since the reset (the CRNN's cache counts these)
  int par = 0;
  int tick(int flags, int &np) {  // returns frames completed
    int nf = 0;
    np = 0;
    if (flags & 2) return 0;  // an active stream is not sampled at all
    for (int i = 0; i < 320; ++i) {
      ++buffered;
      if (buffered == 512) {
        ++nf;
        buffered -= 160;
      }
    }
    if (flags & 1) np = nf;
    return nf;
  }
};

static void run_script(int S, int K, sa_form form) {
  const int T = 151, R = T + 1, HR = 2 * R, GXC = 144, V = S * K;
  std::vector<int> fill(S, 0), pos(S, 0), rowq(S, 0), par(S, 0), expect;
  std::vector<int32_t> ctl((size_t)S * 4), valid((size_t)2 * V + 1, -7), aux((size_t)2 * V + 1, -7), n_post(S);
  std::vector<int64_t> row((size_t)2 * V + 1, -7);
  std::vector<model_stream> ms(S);
  std::vector<float> post((size_t)V * 2);
  bool saw[3] = {false, false, false};
  for (int tick = 0; tick < 700; ++tick) {
    if (tick % 97 == 50) {  // a reset of a random stream, as ww_stream_reset leaves the mirrors (the parity stays)
      const int s = (int)rnd(S);
      fill[s] = pos[s] = rowq[s] = 0;
      ms[s].buffered = 0; ms[s].rows = 0; ms[s].posts = 0;
    }
    sa_tick tk;
    tk.S = S; tk.K = K; tk.T = T; tk.HR = HR; tk.gxc = GXC; tk.form = form;
    tk.fill = fill.data(); tk.pos = pos.data(); tk.rowq = rowq.data(); tk.par = par.data();
    tk.ctl = ctl.data(); tk.row = row.data(); tk.valid = valid.data(); tk.aux = aux.data();
    tk.expect = &expect;
    expect.clear();
    int nd_ref = 0, nw_ref = 0;
    std::vector<int> expect_ref;
    for (int s = 0; s < S; ++s) {
      // every mix of the two bits, weighted towards speech; the first ticks all speech so that rings fill
      const int flags = tick % 7 == 3 ? (int)rnd(4) : (rnd(10) < 8 ? 1 : 0) | (rnd(10) < 1 ? 2 : 0);
      const int fill0 = ms[s].buffered, pos0 = (int)(form == SA_CAUSAL ? ms[s].rows % R : ms[s].posts % R), q0 = (int)(ms[s].posts % GXC),
                par0 = ms[s].par;
      int np_ref = 0;
      const int nf_ref = ms[s].tick(flags, np_ref);
      n_post[s] = sa_tick_stream(tk, s, flags | (int)(rnd(2) << 4));  // (bits above the two are the caller's own: ignored)
      CHECK(n_post[s] == np_ref && np_ref <= 2 && nf_ref <= 2);
      saw[np_ref] = true;
      // ---- control words
      CHECK(ctl[s * 4 + 0] == fill0 && ctl[s * 4 + 1] == nf_ref);
      if (form == SA_ONE_LAUNCH) {
        CHECK(ctl[s * 4 + 2] == (flags | (par0 << 2)) && ctl[s * 4 + 3] == (pos0 | (q0 << 16)));
        if (!(flags & 2)) ms[s].par ^= 1;
        CHECK(par[s] == ms[s].par);
      } else if (form == SA_CAUSAL) {
        CHECK(ctl[s * 4 + 2] == (flags | 1) && ctl[s * 4 + 3] == pos0);
      } else {
        CHECK(ctl[s * 4 + 2] == flags && ctl[s * 4 + 3] == pos0);
      }
      // ---- descriptors and tag slots of the K virtual streams
      for (int j = 0; j < K; ++j) {
        const int v = s * K + j;
        CHECK(sa_virtual(s, K, j) == v && sa_stream(v, K) == s && sa_slot(v, K) == j);
        if (form == SA_ONE_LAUNCH) {
          for (int k = 0; k < np_ref; ++k) expect_ref.push_back(2 * v + k);
        } else if (form == SA_CAUSAL) {
          if (nf_ref) {
            CHECK(nd_ref < 2 * V);
            CHECK(row[nd_ref] == (int64_t)s * HR + pos0 && valid[nd_ref] == nf_ref && aux[nd_ref] == (v | ((np_ref ? 1 : 0) << 16)));
            CHECK(pos0 + nf_ref - 1 <= R && (aux[nd_ref] & 0xffff) == v);  // (rows pos, pos + 1 of a mirrored ring of 2 R rows)
            ++nd_ref;
          }
          for (int k = 0; k < np_ref; ++k) expect_ref.push_back(2 * v + k);
        } else {
          for (int k = 0; k < np_ref; ++k) {
            CHECK(nd_ref < 2 * V);
            // the window that ends at the stream's row (rows + k): T rows from slot (that row + 2) % R of the PHYSICAL stream's ring
            CHECK(row[nd_ref] == (int64_t)s * HR + (pos0 + k + 2) % R && row[nd_ref] + T <= (int64_t)(s + 1) * HR);
            CHECK(valid[nd_ref] == T);
            CHECK(aux[nd_ref] == v * GXC + (q0 + k + 1) % GXC && aux[nd_ref] / GXC == v);
            expect_ref.push_back(nd_ref);
            ++nd_ref;
          }
        }
      }
      nw_ref += np_ref * K;
      ms[s].rows += nf_ref;
      ms[s].posts += np_ref;
      CHECK(fill[s] == ms[s].buffered && fill[s] <= 511);
      CHECK(pos[s] == (int)((form == SA_CAUSAL ? ms[s].rows : ms[s].posts) % R) && rowq[s] == (int)(ms[s].posts % GXC));
    }
    CHECK(tk.nw == nw_ref && tk.nd == nd_ref && expect == expect_ref && (int)expect.size() == nw_ref);
    CHECK(row[2 * V] == -7 && valid[2 * V] == -7 && aux[2 * V] == -7);  // nothing past the tables
    std::set<int> once(expect.begin(), expect.end());
    CHECK(once.size() == expect.size());
    for (int e : expect) CHECK(e >= 0 && e < 2 * V);
    // ---- the scatter: what arrived in slot i is the float i + 1
    for (float &p : post) p = -1.f;
    sa_scatter(form, S, K, n_post.data(), [&](int slot) {
      CHECK(once.count(slot) == 1);
      return (float)(slot + 1);
    }, post.data());
    int w = 0;
    for (int s = 0; s < S; ++s)
      for (int j = 0; j < K; ++j)
        for (int k = 0; k < 2; ++k) {
          const float got = post[((size_t)s * K + j) * 2 + k];
          if (k >= n_post[s]) CHECK(got == 0.f);
          else CHECK(got == (float)((form == SA_TABLE ? w++ : 2 * (s * K + j) + k) + 1));
        }
  }
  CHECK(saw[0] && saw[1] && saw[2]);
  for (int s = 0; s < S; ++s) CHECK(ms[s].rows > 0);
}

int main() {
  char why[320] = {0};
  const int Ks[] = {1, 3, 5}, Ss[] = {1, 5};
  for (int K : Ks)
    for (int S : Ss)
      for (int f = 0; f < 3; ++f) run_script(S, K, (sa_form)f);

  // ---- the member table and the virtual ids of a reset
  std::vector<int32_t> ids;
  const int32_t mem[3] = {2, 0, 2};
  sa_member_table(mem, 3, 5, ids);
  CHECK(ids.size() == 15);
  for (int v = 0; v < 15; ++v) CHECK(ids[v] == mem[v % 3]);
  sa_member_table(nullptr, 4, 2, ids);
  CHECK(ids.size() == 8);
  for (int v = 0; v < 8; ++v) CHECK(ids[v] == v % 4);
  const int32_t named[3] = {4, 0, 4};
  std::vector<int32_t> vids;
  sa_virtual_ids(named, 3, 3, vids);
  const int32_t want_v[9] = {12, 13, 14, 0, 1, 2, 12, 13, 14};
  CHECK(vids.size() == 9 && memcmp(vids.data(), want_v, sizeof want_v) == 0);
  sa_virtual_ids(nullptr, 2, 2, vids);
  CHECK(vids.size() == 4 && vids[0] == 0 && vids[1] == 1 && vids[2] == 2 && vids[3] == 3);

  // ---- refusals of a creation, each with its reason
  CHECK(sa_check_create(5, 3, 0, why, sizeof why) == WW_OK);
  CHECK(sa_check_create(5, 3, WW_STREAM_TWO_LAUNCH | WW_STREAM_SYNC_WAIT | WW_STREAM_CAUSAL, why, sizeof why) == WW_OK);
  CHECK(sa_check_create(1, 64, 0, why, sizeof why) == WW_OK);
  CHECK(sa_check_create(21845, 3, 0, why, sizeof why) == WW_OK);  // 65535 virtual streams
  why[0] = 0;
  CHECK(sa_check_create(5, 0, 0, why, sizeof why) == WW_EINVAL && strstr(why, "1..64"));
  CHECK(sa_check_create(5, 65, 0, why, sizeof why) == WW_EINVAL && strstr(why, "65 member slots"));
  CHECK(sa_check_create(5, -1, 0, why, sizeof why) == WW_EINVAL && strstr(why, "member slots"));
  CHECK(sa_check_create(5, 3, WW_STREAM_FULL_RECOMPUTE, why, sizeof why) == WW_EINVAL && strstr(why, "WW_STREAM_FULL_RECOMPUTE"));
  CHECK(sa_check_create(5, 3, 64u, why, sizeof why) == WW_EINVAL && strstr(why, "0x40"));
  CHECK(sa_check_create(0, 3, 0, why, sizeof why) == WW_EINVAL && strstr(why, "stream count"));
  CHECK(sa_check_create(16384, 4, 0, why, sizeof why) == WW_EINVAL && strstr(why, "65536 virtual streams"));
  CHECK(sa_check_create(65535, 2, 0, why, sizeof why) == WW_EINVAL && strstr(why, "131070"));
  CHECK(sa_check_create(2147483647, 64, 0, why, sizeof why) == WW_EINVAL);  // (no overflow on the way)
  CHECK(sa_check_create(5, 3, 0, nullptr, 0) == WW_OK && sa_check_create(5, 0, 0, nullptr, 0) == WW_EINVAL);

  // ---- refusals of a call on the wrong kind of bank
  const char *not_on_every[] = {"ww_stream_step", "ww_stream_step_trigger", "ww_pipeline_bank_step", "ww_stream_set_model", "ww_stream_feed",
                                "ww_stream_feed_rows"};
  for (const char *c : not_on_every) {
    why[0] = 0;
    CHECK(sa_check_call(true, c, false, why, sizeof why) == WW_EINVAL && strstr(why, c) == why && strstr(why, "ww_stream_step_all"));
    CHECK(sa_check_call(false, c, false, why, sizeof why) == WW_OK);
  }
  why[0] = 0;
  CHECK(sa_check_call(false, "ww_stream_step_all", true, why, sizeof why) == WW_EINVAL && strstr(why, "ww_stream_create_set_all"));
  CHECK(sa_check_call(true, "ww_stream_step_all", true, why, sizeof why) == WW_OK);
  char tiny[8];
  CHECK(sa_check_call(true, "ww_stream_step", false, tiny, sizeof tiny) == WW_EINVAL && strlen(tiny) == 7);  // cut, not overrun

  // ---- the id list of a reset or a move on a bank of 4 streams: each refusal alone, then two at once in the fixed order
  {
    const int S = 4;
    const int32_t good[8] = {0, 3, 3, 1, 2, 0, 3, 3}, low[3] = {0, -1, 2}, high[3] = {0, 1, 4}, nine[9] = {0, 1, 2, 3, 0, 1, 2, 3, 0};
    CHECK(sa_check_ids(nullptr, 0, S, why, sizeof why) == WW_OK);
    CHECK(sa_check_ids(nullptr, -5, S, why, sizeof why) == WW_OK && sa_check_ids(nullptr, 1000, S, why, sizeof why) == WW_OK);  // every stream: n is not looked at
    CHECK(sa_check_ids(good, 0, S, why, sizeof why) == WW_OK);
    CHECK(sa_check_ids(good, 3, S, why, sizeof why) == WW_OK);
    CHECK(sa_check_ids(good, 2 * S, S, why, sizeof why) == WW_OK);  // a stream may be named again: up to 2 S ids
    why[0] = 0;
    CHECK(sa_check_ids(good, -1, S, why, sizeof why) == WW_EINVAL && strcmp(why, "negative id count") == 0);
    CHECK(sa_check_ids(nine, 2 * S + 1, S, why, sizeof why) == WW_EINVAL && strcmp(why, "more ids than streams") == 0);
    CHECK(sa_check_ids(low, 3, S, why, sizeof why) == WW_EINVAL && strcmp(why, "stream id -1 out of range") == 0);
    CHECK(sa_check_ids(high, 3, S, why, sizeof why) == WW_EINVAL && strcmp(why, "stream id 4 out of range") == 0);
    CHECK(sa_check_ids(high, 2, S, why, sizeof why) == WW_OK);  // (the bad id lies behind the count)
    const int32_t nine_bad[9] = {7, 1, 2, 3, 0, 1, 2, 3, 0};
    CHECK(sa_check_ids(nine_bad, 9, S, why, sizeof why) == WW_EINVAL && strstr(why, "more ids"));  // the count is looked at before the ids
    CHECK(sa_check_ids(good, 1, 0, why, sizeof why) == WW_EINVAL && strstr(why, "more ids"));
    CHECK(sa_check_ids(low, 3, S, nullptr, 0) == WW_EINVAL);
  }

  printf("ok %ld\n", n_checks);
  return 0;
}
