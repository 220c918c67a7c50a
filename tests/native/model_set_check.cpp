// model_set_check - csrc/model_set.h (the host half of ww_model_set) alone on the CPU, under Address + UB sanitizer
// (tests/test_model_set_host.py compiles and runs it; nothing here touches a GPU).  Over synthetic packed models:
//   * ww_set_check accepts equal members and refuses, each with a message, a member of another context, another kind, a split-bf16
//     member, a generic CRNN, every single field of ww_model_info / ww_crnn_geom / ww_wave_geom / ww_filter_geom one off (the
//     Wavenet's dilations, block order and has_res included), another block size, one byte of the filter off, 0 and 65 members;
//   * ww_set_stride rounds up to 256 and never down;
//   * ww_set_translate_model moves EVERY pointer of ww_filter_dev / ww_crnn_dev / ww_wave_dev to the same offset of the set's
//     block, keeps nullptr, stays inside [set block, set block + block size) and refuses a pointer outside the member's block;
//   * ww_set_check_ids accepts 0 .. K - 1 and nullptr, refuses -1 and K and says where.
// Prints "ok <checks>" and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <type_traits>
#include <utility>

#include "model_pack.h"
#include "model_set.h"

static int n_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++n_checks;                                                            \
    if (!(cond)) {                                                         \
      fprintf(stderr, "model_set_check: %s (line %d)\n", #cond, __LINE__); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

// a synthetic packed model: geometry by hand, arrays of a few bytes each under the packer's names
static ww_packed_model make_model(int kind, unsigned seed) {
  ww_packed_model pm;
  pm.kind = kind;
  pm.filt.n_mel = 40; pm.filt.n_bins = 257; pm.filt.floor_v = 1e-3f; pm.filt.log_off = 0.5f; pm.filt.scale = 2.0f;
  pm.filt.total_taps = 500; pm.filt.max_len = 36; pm.filt.melv_aligned = 1;
  pm.info = {kind, kind == WW_KIND_CRNN ? 151 : 182, 40, 257, 2, kind == WW_KIND_CRNN ? 1 : 182, kind == WW_KIND_CRNN ? 64 : 32, 0};
  std::vector<float> filt_a(300), filt_b(77);
  for (size_t i = 0; i < filt_a.size(); ++i) filt_a[i] = (float)i * 0.25f;  // the filter does not depend on the seed
  for (size_t i = 0; i < filt_b.size(); ++i) filt_b[i] = (float)i - 3.0f;
  std::vector<double> hann(64, 0.5);
  pm.add("filt.wdense", filt_a); pm.add("filt.bias", filt_b); pm.add("filt.hann", hann);
  std::vector<float> w(1000 + 7);
  for (size_t i = 0; i < w.size(); ++i) w[i] = (float)((i * 2654435761u + seed) % 1000) * 1e-3f;  // the weights do
  if (kind == WW_KIND_CRNN) {
    pm.crnn.n_mel = 40; pm.crnn.T = 151; pm.crnn.C = 32; pm.crnn.KF = 5; pm.crnn.KT = 20; pm.crnn.SF = 2; pm.crnn.ST = 8; pm.crnn.PF = 1;
    pm.crnn.PT = 6; pm.crnn.OF = 20; pm.crnn.OT = 19; pm.crnn.H = 32; pm.crnn.NOUT = 2; pm.crnn.HEAD = 1; pm.crnn.generic = false; pm.crnn.FEATP = 640;
    pm.add("crnn.conv_w", w); pm.add("crnn.wx1s", w); pm.add("crnn.b2", w);
  } else {
    pm.wave.T = 182; pm.wave.n_mel = 40; pm.wave.C = 16; pm.wave.S = 32; pm.wave.NB = 4; pm.wave.NOUT = 2;
    pm.wave.dil = {1, 2, 4, 8}; pm.wave.order = {0, 1, 2, 3}; pm.wave.has_res = {1, 1, 1, 0};
    pm.add("wave.w_in", w); pm.add("wave.w_gate", w); pm.add("wave.d_b2", w);
  }
  return pm;
}

struct member_box {
  ww_packed_model pm;
  std::vector<uint8_t> image;
  int precision = WW_PRECISION_FP32;
  const void *ctx = nullptr;
  size_t block_bytes = 0;
  ww_set_member view() const {
    ww_set_member m;
    m.ctx = ctx; m.kind = pm.kind; m.precision = precision; m.info = pm.info;
    m.filt = &pm.filt; m.crnn = &pm.crnn; m.wave = &pm.wave;
    m.block_bytes = block_bytes; m.filt_image = &image;
    return m;
  }
};
static member_box box_of(int kind, unsigned seed, const void *ctx) {
  member_box b;
  b.pm = make_model(kind, seed);
  b.image = ww_set_filter_image(b.pm.table, b.pm.bytes.data());
  b.ctx = ctx;
  b.block_bytes = b.pm.bytes.size();
  return b;
}

static int check3(const member_box &a, const member_box &b, const member_box &c, const void *ctx, std::string *why = nullptr) {
  const ww_set_member mem[3] = {a.view(), b.view(), c.view()};
  char err[384] = {0};
  const int rc = ww_set_check(mem, 3, ctx, err, sizeof err);
  if (why) *why = err;
  CHECK((rc == WW_OK) == (err[0] == 0));  // a refusal always says why
  return rc;
}

// member 2 with one thing changed must be refused, and the message must hold `word`
static void refuse_one_off(int kind, const void *ctx, const char *word, const std::function<void(member_box &)> &change) {
  member_box a = box_of(kind, 1, ctx), b = box_of(kind, 2, ctx), c = box_of(kind, 3, ctx);
  CHECK(check3(a, b, c, ctx) == WW_OK);
  change(c);
  std::string why;
  CHECK(check3(a, b, c, ctx, &why) == WW_EINVAL);
  if (why.find(word) == std::string::npos) {
    fprintf(stderr, "model_set_check: refusal \"%s\" does not mention \"%s\"\n", why.c_str(), word);
    exit(1);
  }
  CHECK(why.find("member 2") != std::string::npos);
}

int main() {
  int ctx_a = 0, ctx_b = 0;
  const void *ctx = &ctx_a;
  for (int kind : {WW_KIND_CRNN, WW_KIND_WAVENET}) {
    // equal geometry, different weights: one set; the weights are no part of the filter image
    member_box a = box_of(kind, 1, ctx), b = box_of(kind, 2, ctx);
    CHECK(a.image == b.image && a.pm.bytes != b.pm.bytes && a.block_bytes == b.block_bytes);
    CHECK(check3(a, b, a, ctx) == WW_OK);
    refuse_one_off(kind, ctx, "context", [&](member_box &m) { m.ctx = &ctx_b; });
    refuse_one_off(kind, ctx, "bf16", [](member_box &m) { m.precision = WW_PRECISION_BF16X3; });
    refuse_one_off(kind, ctx, "kind", [&](member_box &m) { m.pm.kind = kind == WW_KIND_CRNN ? WW_KIND_WAVENET : WW_KIND_CRNN; });
    refuse_one_off(kind, ctx, "kind", [](member_box &m) { m.pm.kind = 7; });
    // every field of the info
    int32_t ww_model_info::*info_fields[] = {&ww_model_info::kind, &ww_model_info::window, &ww_model_info::n_mel, &ww_model_info::n_bins,
                                             &ww_model_info::n_out, &ww_model_info::enc_rows, &ww_model_info::enc_width, &ww_model_info::reserved};
    for (auto f : info_fields) refuse_one_off(kind, ctx, "info", [f](member_box &m) { m.pm.info.*f += 1; });
    // every field of the filter's geometry, and one byte of its arrays (first, middle, last)
    int ww_filter_geom::*fi[] = {&ww_filter_geom::n_mel, &ww_filter_geom::n_bins, &ww_filter_geom::total_taps, &ww_filter_geom::max_len, &ww_filter_geom::melv_aligned};
    for (auto f : fi) refuse_one_off(kind, ctx, "filter", [f](member_box &m) { m.pm.filt.*f += 1; });
    float ww_filter_geom::*ff[] = {&ww_filter_geom::floor_v, &ww_filter_geom::log_off, &ww_filter_geom::scale};
    for (auto f : ff) refuse_one_off(kind, ctx, "filter", [f](member_box &m) { m.pm.filt.*f *= 1.0000002f; });
    const size_t img = a.image.size();
    for (size_t at : {size_t(0), img / 2, img - 1}) refuse_one_off(kind, ctx, "filter", [at](member_box &m) { m.image[at] ^= 1; });
    refuse_one_off(kind, ctx, "filter", [](member_box &m) { m.image.push_back(0); });
    refuse_one_off(kind, ctx, "bytes", [](member_box &m) { m.block_bytes += 256; });
  }
  {  // the geometries, field by field
    int ww_crnn_geom::*ci[] = {&ww_crnn_geom::n_mel, &ww_crnn_geom::T, &ww_crnn_geom::C, &ww_crnn_geom::KF, &ww_crnn_geom::KT, &ww_crnn_geom::SF,
                               &ww_crnn_geom::ST, &ww_crnn_geom::PF, &ww_crnn_geom::PT, &ww_crnn_geom::OF, &ww_crnn_geom::OT, &ww_crnn_geom::H,
                               &ww_crnn_geom::NOUT, &ww_crnn_geom::HEAD, &ww_crnn_geom::FEATP};
    for (auto f : ci) refuse_one_off(WW_KIND_CRNN, ctx, "geometry", [f](member_box &m) { m.pm.crnn.*f += 1; });
    refuse_one_off(WW_KIND_CRNN, ctx, "generic", [](member_box &m) { m.pm.crnn.generic = true; });
    int ww_wave_geom::*wi[] = {&ww_wave_geom::T, &ww_wave_geom::n_mel, &ww_wave_geom::C, &ww_wave_geom::S, &ww_wave_geom::NB, &ww_wave_geom::NOUT};
    for (auto f : wi) refuse_one_off(WW_KIND_WAVENET, ctx, "geometry", [f](member_box &m) { m.pm.wave.*f += 1; });
    refuse_one_off(WW_KIND_WAVENET, ctx, "dilations", [](member_box &m) { m.pm.wave.dil[2] = 2; });
    refuse_one_off(WW_KIND_WAVENET, ctx, "block order", [](member_box &m) { std::swap(m.pm.wave.order[0], m.pm.wave.order[1]); });
    refuse_one_off(WW_KIND_WAVENET, ctx, "residual", [](member_box &m) { m.pm.wave.has_res[3] = 1; });
    refuse_one_off(WW_KIND_WAVENET, ctx, "geometry", [](member_box &m) { m.pm.wave.order_is_natural = false; });
    // a CRNN's wave geometry (and a Wavenet's CRNN geometry) is no part of the comparison
    member_box a = box_of(WW_KIND_CRNN, 1, ctx), b = box_of(WW_KIND_CRNN, 2, ctx);
    b.pm.wave.dil = {3};
    CHECK(check3(a, b, a, ctx) == WW_OK);
  }
  {  // the member count
    member_box a = box_of(WW_KIND_CRNN, 1, ctx);
    std::vector<ww_set_member> many(WW_SET_MAX_MODELS + 1, a.view());
    char err[256];
    CHECK(ww_set_check(many.data(), 0, ctx, err, sizeof err) == WW_EINVAL);
    CHECK(ww_set_check(many.data(), -1, ctx, err, sizeof err) == WW_EINVAL);
    CHECK(ww_set_check(many.data(), WW_SET_MAX_MODELS + 1, ctx, err, sizeof err) == WW_EINVAL);
    CHECK(ww_set_check(many.data(), WW_SET_MAX_MODELS, ctx, err, sizeof err) == WW_OK);
    CHECK(ww_set_check(many.data(), 1, ctx, err, sizeof err) == WW_OK);
    CHECK(ww_set_check(nullptr, 2, ctx, err, sizeof err) == WW_EINVAL);
    CHECK(ww_set_check(many.data(), 2, ctx, nullptr, 0) == WW_OK);  // (no room for a message is no crash)
    many[1].filt_image = nullptr;
    CHECK(ww_set_check(many.data(), 2, ctx, nullptr, 0) == WW_EINVAL);
  }
  // ---- the stride
  CHECK(ww_set_stride(1) == 256 && ww_set_stride(256) == 256 && ww_set_stride(257) == 512 && ww_set_stride(0) == 0);
  for (size_t b = 1; b < 5000; b += 37) CHECK(ww_set_stride(b) >= b && ww_set_stride(b) - b < WW_SET_ALIGN && ww_set_stride(b) % WW_SET_ALIGN == 0);
  // ---- the translation: member 0's block at one address, the set's at another; every pointer moves by the same distance
  for (int kind : {WW_KIND_CRNN, WW_KIND_WAVENET}) {
    const size_t bytes = 40 * 256, K = 3, stride = ww_set_stride(bytes);
    std::vector<uint8_t> member(bytes), set(K * stride);
    ww_filter_dev f;
    ww_crnn_dev c;
    ww_wave_dev v;
    // every pointer of the three structs at an offset of its own inside the member's block (those of the other kind stay nullptr)
    size_t at = 0, n_ptr = 0;
    auto place = [&](auto *&p) {
      p = (std::remove_reference_t<decltype(p)>)(member.data() + at);
      at += 256;
      ++n_ptr;
    };
    ww_set_each_pointer(f, place);
    if (kind == WW_KIND_CRNN) ww_set_each_pointer(c, place);
    else ww_set_each_pointer(v, place);
    CHECK(n_ptr == (kind == WW_KIND_CRNN ? 10u + 21u : 10u + 13u) && at <= bytes);
    ww_filter_dev f0 = f;
    ww_crnn_dev c0 = c;
    ww_wave_dev v0 = v;
    CHECK(ww_set_translate_model(f, c, v, member.data(), bytes, set.data()));
    size_t seen = 0;
    auto walk = [&](auto &now, auto &before) {
      std::vector<const void *> was;
      ww_set_each_pointer(before, [&](auto *&p) { was.push_back(p); });
      size_t i = 0;
      ww_set_each_pointer(now, [&](auto *&p) {
        const void *w = was[i++];
        if (!w) {
          CHECK(p == nullptr);
          return;
        }
        const uint8_t *q = (const uint8_t *)p;
        CHECK(q >= set.data() && q < set.data() + bytes);                                  // inside member 0's copy
        CHECK((size_t)(q - set.data()) == (size_t)((const uint8_t *)w - member.data()));   // at the offset it had
        for (size_t k = 0; k < K; ++k) CHECK(q + k * stride + 256 <= set.data() + set.size());  // and member k's copy inside the set
        ++seen;
      });
    };
    walk(f, f0); walk(c, c0); walk(v, v0);
    CHECK(seen == n_ptr);
    // a pointer outside the member's block (one byte behind it, one in front of it) is refused and left alone
    ww_filter_dev g = f0;
    g.bias = (float *)(member.data() + bytes);
    ww_crnn_dev c1 = c0;
    ww_wave_dev v1 = v0;
    CHECK(!ww_set_translate_model(g, c1, v1, member.data(), bytes, set.data()));
    CHECK((const uint8_t *)g.bias == member.data() + bytes);
    float *lone = (float *)(member.data() + 512);
    CHECK(!ww_set_translate(lone, member.data() + 516, bytes - 516, set.data()) && (uint8_t *)lone == member.data() + 512);
    float *none = nullptr;
    CHECK(ww_set_translate(none, member.data(), bytes, set.data()) && none == nullptr);
  }
  {  // ---- member ids
    char err[160] = {0};
    const int32_t good[] = {0, 2, 1, 2, 0}, low[] = {0, -1, 1}, high[] = {0, 1, 3};
    CHECK(ww_set_check_ids(good, 5, 3, "win_model", err, sizeof err) == WW_OK && err[0] == 0);
    CHECK(ww_set_check_ids(nullptr, 5, 3, "stream_model", err, sizeof err) == WW_OK);
    CHECK(ww_set_check_ids(good, 0, 3, "win_model", err, sizeof err) == WW_OK);
    CHECK(ww_set_check_ids(low, 3, 3, "win_model", err, sizeof err) == WW_EINVAL && strstr(err, "win_model[1] = -1"));
    CHECK(ww_set_check_ids(high, 3, 3, "stream_model", err, sizeof err) == WW_EINVAL && strstr(err, "stream_model[2] = 3"));
    CHECK(ww_set_check_ids(high, 2, 3, "stream_model", err, sizeof err) == WW_OK);  // (only the entries the call names)
    CHECK(ww_set_check_ids(good, 5, 2, "win_model", nullptr, 0) == WW_EINVAL);
  }
  printf("ok %d checks\n", n_checks);
  return 0;
}
