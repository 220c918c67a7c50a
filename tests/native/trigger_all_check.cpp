// trigger_all_check - the trigger rule of csrc/stream_all.h (sa_trigger_update: the wake-word stage with K member slots per stream,
// which says WHICH wake word fired) alone on the CPU, under Address + UB sanitizer (tests/test_trigger_all_host.py compiles and runs
// it; nothing here touches a GPU).  Over S in {1, 7} streams and K in {1, 2, 3, 64} slots, 400 ticks of seeded random posteriors,
// row counts and flags are held against a restatement written the way the reference runs (spokestack/wakeword/tflite.py:134-146,
// 232-239: one stream, one row, one slot at a time, with a list of the slots that exceeded per row):
//   * posterior_max per slot, cleared for all K slots on the VAD falling edge, behind the tick's rows;
//   * a stream fires once when any slot exceeds on any row and it is not active; an active stream is not listed and its maxima move;
//   * fired_mask = the slots that exceeded on any row of the tick; fired_slot = on the EARLIEST row with an exceeding slot, the one
//     with the greatest posterior, the lowest slot among equals;
//   * fall_ids, with and without a fire in the same tick; n_post of 0, 1 and 2.
// Posteriors and thresholds come from nine values (k / 8), so ties between slots, slots exceeding on different rows of one tick and
// posteriors EQUAL to a threshold (which do not exceed) all occur - the program counts them and fails if a case never arose.
// Then directed cases of each, K = 1 against the one-threshold statement, and every refusal of sa_check_trigger.
// Prints "ok <checks>" and exits 0; or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stream_all.h"

static long n_checks = 0;
#define CHECK(cond)                                                             \
  do {                                                                          \
    ++n_checks;                                                                 \
    if (!(cond)) {                                                              \
      fprintf(stderr, "trigger_all_check: %s (line %d)\n", #cond, __LINE__);   \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)

static unsigned long long rng_state = 0x2545f4914f6cdd1dull;
static unsigned rnd(unsigned n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)((rng_state >> 33) % n);
}

// what arose
static long c_tie = 0, c_two_rows = 0, c_active_exceeds = 0, c_fall_fire = 0, c_fall_alone = 0, c_np[3] = {0, 0, 0}, c_equal_thr = 0, c_fires = 0;

// one stream of the restatement: the reference's stage object, with a maximum per wake word
struct ref_stream {
  bool was_speech = false;
  std::vector<float> pmax;
  // one tick: returns true when the stream fires; winner and mask are then set
  bool tick(int K, bool speech, bool &active, const float *post /*[K][2]*/, int np, const double *thr, int &winner, uint64_t &mask, bool &fall) {
    fall = was_speech && !speech;
    was_speech = speech;
    bool any = false;
    winner = -1;
    mask = 0;
    int rows_with = 0;
    for (int row = 0; row < np; ++row) {
      std::vector<int> over;  // the slots that exceed on this row
      for (int j = 0; j < K; ++j) {
        const float p = post[j * 2 + row];
        if (p > pmax[(size_t)j]) pmax[(size_t)j] = p;
        if ((double)p == thr[j]) ++c_equal_thr;
        if ((double)p > thr[j]) over.push_back(j);
      }
      if (over.empty()) continue;
      ++rows_with;
      for (int j : over) mask |= (uint64_t)1 << j;
      if (!any) {  // the earliest such row names the winner
        any = true;
        float top = post[over[0] * 2 + row];
        for (int j : over) top = post[j * 2 + row] > top ? post[j * 2 + row] : top;
        int ties = 0;
        for (int j : over)
          if (post[j * 2 + row] == top) {
            if (winner < 0) winner = j;
            ++ties;
          }
        if (ties > 1) ++c_tie;
      }
    }
    if (rows_with == 2) ++c_two_rows;
    bool fired = false;
    if (any && active) ++c_active_exceeds;
    if (any && !active) {
      active = true;
      fired = true;
    }
    if (fall) {
      for (float &m : pmax) m = 0.f;
      ++(fired ? c_fall_fire : c_fall_alone);
    }
    return fired;
  }
};

static void random_run(int S, int K, int ticks) {
  std::vector<ref_stream> ref((size_t)S);
  for (ref_stream &r : ref) r.pmax.assign((size_t)K, 0.f);
  std::vector<uint8_t> speech((size_t)S), active((size_t)S, 0), ref_active((size_t)S, 0), was((size_t)S, 0);
  std::vector<float> post((size_t)S * K * 2), pmax((size_t)S * K, 0.f);
  std::vector<int32_t> np((size_t)S), fired((size_t)S), slot((size_t)S), fall((size_t)S);
  std::vector<uint64_t> mask((size_t)S);
  std::vector<double> thr((size_t)K);
  for (int j = 0; j < K; ++j) thr[(size_t)j] = (4 + rnd(4)) / 8.0;  // 0.5 .. 0.875
  for (int t = 0; t < ticks; ++t) {
    for (int s = 0; s < S; ++s) {
      speech[(size_t)s] = rnd(8) != 0 ? 2 : 0;  // (any non-zero byte is "speech")
      np[(size_t)s] = (int32_t)rnd(3);
      ++c_np[np[(size_t)s]];
      if (rnd(6) == 0) active[(size_t)s] = ref_active[(size_t)s] = 0;  // the timeout stage
      // mostly quiet posteriors, so that streams are often inactive when a slot exceeds
      for (int i = 0; i < K * 2; ++i) post[(size_t)s * K * 2 + i] = rnd(K > 8 ? 40 : 4) == 0 ? rnd(9) / 8.0f : rnd(4) / 8.0f;
    }
    int32_t nf = -1, nl = -1;
    std::fill(fired.begin(), fired.end(), -9);
    std::fill(slot.begin(), slot.end(), -9);
    std::fill(mask.begin(), mask.end(), ~0ull);
    std::fill(fall.begin(), fall.end(), -9);
    sa_trigger_update(S, K, speech.data(), active.data(), post.data(), np.data(), thr.data(), was.data(), pmax.data(), fired.data(), slot.data(),
                      mask.data(), &nf, fall.data(), &nl);
    int wf = 0, wl = 0;
    for (int s = 0; s < S; ++s) {
      bool a = ref_active[(size_t)s] != 0, fl = false;
      int w = -1;
      uint64_t m = 0;
      const bool f = ref[(size_t)s].tick(K, speech[(size_t)s] != 0, a, post.data() + (size_t)s * K * 2, np[(size_t)s], thr.data(), w, m, fl);
      ref_active[(size_t)s] = a;
      if (f) {
        ++c_fires;
        CHECK(wf < nf && fired[(size_t)wf] == s && slot[(size_t)wf] == w && mask[(size_t)wf] == m && ((m >> w) & 1));
        ++wf;
      }
      if (fl) {
        CHECK(wl < nl && fall[(size_t)wl] == s);
        ++wl;
      }
      CHECK(active[(size_t)s] == (a ? 1 : 0) && was[(size_t)s] == (speech[(size_t)s] ? 1 : 0));
      for (int j = 0; j < K; ++j) CHECK(pmax[(size_t)s * K + j] == ref[(size_t)s].pmax[(size_t)j]);
    }
    CHECK(wf == nf && wl == nl);
    for (int i = nf; i < S; ++i) CHECK(fired[(size_t)i] == -9 && slot[(size_t)i] == -9 && mask[(size_t)i] == ~0ull);  // nothing behind the lists
    for (int i = nl; i < S; ++i) CHECK(fall[(size_t)i] == -9);
  }
}

// one stream, K slots, one tick from a clean state
struct one_tick {
  int32_t nf = 0, nl = 0, fired = -1, slot = -1, fall = -1;
  uint64_t mask = 0;
  std::vector<float> pmax;
  uint8_t active = 0, was = 0;
};
static one_tick run_one(int K, std::vector<float> post, int np, std::vector<double> thr, uint8_t speech, uint8_t active, uint8_t was, float pmax0 = 0.f) {
  one_tick o;
  o.pmax.assign((size_t)K, pmax0);
  o.active = active;
  o.was = was;
  const int32_t n = np;
  sa_trigger_update(1, K, &speech, &o.active, post.data(), &n, thr.data(), &o.was, o.pmax.data(), &o.fired, &o.slot, &o.mask, &o.nf, &o.fall, &o.nl);
  return o;
}

int main() {
  for (int S : {1, 7})
    for (int K : {1, 2, 3, 64}) random_run(S, K, 400);
  CHECK(c_tie > 20 && c_two_rows > 20 && c_active_exceeds > 20 && c_fall_fire > 5 && c_fall_alone > 20 && c_equal_thr > 20 && c_fires > 200);
  CHECK(c_np[0] > 100 && c_np[1] > 100 && c_np[2] > 100);

  // ---- directed cases (post is [K][2]: slot j's rows 0 and 1)
  {  // a tie between slots 1 and 2 on row 0: the lowest slot; slot 0 is below its threshold
    one_tick o = run_one(3, {0.4f, 0.f, 0.75f, 0.f, 0.75f, 0.f}, 1, {0.5, 0.5, 0.5}, 1, 0, 1);
    CHECK(o.nf == 1 && o.fired == 0 && o.slot == 1 && o.mask == 6 && o.active == 1 && o.nl == 0);
    CHECK(o.pmax[0] == 0.4f && o.pmax[1] == 0.75f && o.pmax[2] == 0.75f);
  }
  {  // slot 2 exceeds on row 0, slot 0 exceeds higher on row 1: the earliest row wins, the mask has both
    one_tick o = run_one(3, {0.1f, 0.99f, 0.f, 0.f, 0.6f, 0.2f}, 2, {0.5, 0.5, 0.5}, 1, 0, 1);
    CHECK(o.nf == 1 && o.slot == 2 && o.mask == 5 && o.pmax[0] == 0.99f);
  }
  {  // the same with one row delivered: row 1 is not looked at
    one_tick o = run_one(3, {0.1f, 0.99f, 0.f, 0.f, 0.6f, 0.2f}, 1, {0.5, 0.5, 0.5}, 1, 0, 1);
    CHECK(o.nf == 1 && o.slot == 2 && o.mask == 4 && o.pmax[0] == 0.1f);
  }
  {  // no row: nothing fires, whatever post holds
    one_tick o = run_one(2, {0.9f, 0.9f, 0.9f, 0.9f}, 0, {0.5, 0.5}, 1, 0, 1);
    CHECK(o.nf == 0 && o.active == 0 && o.pmax[0] == 0.f && o.fired == -1 && o.slot == -1);
  }
  {  // per-slot thresholds: slot 0's greater posterior is below ITS threshold, a posterior equal to the threshold does not exceed
    one_tick o = run_one(3, {0.8f, 0.f, 0.6f, 0.f, 0.5f, 0.f}, 1, {0.9, 0.5, 0.5}, 1, 0, 1);
    CHECK(o.nf == 1 && o.slot == 1 && o.mask == 2);
  }
  {  // exceeding while already active: not listed, the flag stays, the maxima move
    one_tick o = run_one(2, {0.9f, 0.f, 0.f, 0.f}, 1, {0.5, 0.5}, 1, 1, 1);
    CHECK(o.nf == 0 && o.active == 1 && o.pmax[0] == 0.9f && o.fired == -1);
  }
  {  // a fall with a fire in the same tick: both listed, the maxima cleared behind the rows
    one_tick o = run_one(2, {0.f, 0.f, 0.7f, 0.f}, 1, {0.5, 0.5}, 0, 0, 1, 0.3f);
    CHECK(o.nf == 1 && o.slot == 1 && o.nl == 1 && o.fall == 0 && o.pmax[0] == 0.f && o.pmax[1] == 0.f && o.was == 0);
  }
  {  // a fall without a fire; and no fall where the bit was already down
    one_tick o = run_one(2, {0.2f, 0.f, 0.3f, 0.f}, 1, {0.5, 0.5}, 0, 0, 1, 0.4f);
    CHECK(o.nf == 0 && o.nl == 1 && o.pmax[0] == 0.f && o.pmax[1] == 0.f);
    one_tick q = run_one(2, {0.2f, 0.f, 0.3f, 0.f}, 1, {0.5, 0.5}, 0, 0, 0, 0.4f);
    CHECK(q.nf == 0 && q.nl == 0 && q.pmax[0] == 0.4f && q.pmax[1] == 0.4f);
  }
  {  // slot 63: the mask's top bit
    std::vector<float> post(128, 0.f);
    post[63 * 2] = 0.9f;
    one_tick o = run_one(64, post, 1, std::vector<double>(64, 0.5), 1, 0, 1);
    CHECK(o.nf == 1 && o.slot == 63 && o.mask == (uint64_t)1 << 63);
  }
  {  // K = 1 without the two lists (ww_trigger_bank_step's form)
    uint8_t sp[2] = {1, 0}, act[2] = {0, 0}, was[2] = {1, 1};
    float post[4] = {0.2f, 0.8f, 0.9f, 0.f}, pm[2] = {0.f, 0.5f};
    int32_t np[2] = {2, 1}, fired[2] = {-1, -1}, fall[2] = {-1, -1}, nf = 0, nl = 0;
    const double thr = 0.5;
    sa_trigger_update(2, 1, sp, act, post, np, &thr, was, pm, fired, nullptr, nullptr, &nf, fall, &nl);
    CHECK(nf == 2 && fired[0] == 0 && fired[1] == 1 && nl == 1 && fall[0] == 1 && pm[0] == 0.8f && pm[1] == 0.f && act[0] == 1 && act[1] == 1);
  }

  // ---- refusals
  {
    char why[200];
    uint8_t b[2] = {0, 0};
    float f[8] = {0};
    double thr[2] = {0.5, 0.5};
    int32_t np[2] = {0, 2}, ids[2], n = 0;
    uint64_t m[2];
    auto chk = [&](int64_t S, int64_t K, const void *a0, const int32_t *npp, const void *t, const void *nfp) {
      why[0] = 0;
      return sa_check_trigger(S, K, a0, b, f, npp, t, b, f, ids, ids, m, nfp, ids, &n, why, sizeof why);
    };
    CHECK(chk(2, 2, b, np, thr, &n) == WW_OK && chk(0, 1, nullptr, nullptr, thr, &n) == WW_OK && chk(2, 64, b, np, thr, &n) == WW_OK);
    CHECK(chk(2, 0, b, np, thr, &n) == WW_EINVAL && strstr(why, "member slots"));
    CHECK(chk(2, 65, b, np, thr, &n) == WW_EINVAL && strstr(why, "65 member slots"));
    CHECK(chk(-1, 2, b, np, thr, &n) == WW_EINVAL && strstr(why, "stream count"));
    CHECK(chk(2, 2, nullptr, np, thr, &n) == WW_EINVAL && strstr(why, "NULL"));
    CHECK(chk(2, 2, b, nullptr, thr, &n) == WW_EINVAL && chk(2, 2, b, np, nullptr, &n) == WW_EINVAL && chk(2, 2, b, np, thr, nullptr) == WW_EINVAL);
    int32_t bad[2] = {0, 3}, neg[2] = {-1, 0};
    CHECK(chk(2, 2, b, bad, thr, &n) == WW_EINVAL && strstr(why, "n_post[1] = 3"));
    CHECK(chk(2, 2, b, neg, thr, &n) == WW_EINVAL && strstr(why, "n_post[0] = -1"));
    CHECK(sa_check_trigger(2, 65, b, b, f, np, thr, b, f, ids, ids, m, &n, ids, &n, nullptr, 0) == WW_EINVAL);
  }
  printf("ok %ld\n", n_checks);
  return 0;
}
