// model_pack.h - the host-only half of ww_model_load: parsing a weight blob (wwhip/weights.py: pack_blob) and packing every array a
// kernel reads, in the operand order that kernel reads it, into ONE host buffer with a table of what lies where.  Plain C++ (no HIP
// header, no HIP call): csrc/api.hip includes it and uploads the buffer with one allocation and one copy;
// tests/native/model_pack_check.cpp compiles it alone under Address + UB sanitizer on the CPU (tests/test_host_logic.py) and
// prints a digest per array.  The sizes it shares with the kernels are model_layout.h's.
//
// A blob is read only through memcpy (blob_view::words): neither the caller's buffer nor a section's offset need be aligned.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/wwhip.h"
#include "model_layout.h"

namespace {

#define WW_PACK_ALIGN 256  // every array's offset in the buffer (what each had from an allocation of its own)

struct ww_pack_entry {
  const char *name;
  uint32_t elt;       // bytes per element
  size_t off, bytes;  // in ww_packed_model::bytes
};

struct ww_packed_model {
  int kind = 0;
  ww_model_info info = {};
  ww_filter_geom filt;
  ww_crnn_geom crnn;
  ww_wave_geom wave;
  std::vector<uint8_t> bytes;        // all arrays, each from a multiple of WW_PACK_ALIGN, zeros between them
  std::vector<ww_pack_entry> table;  // in the order they were added
  char err[320] = {0};               // why packing stopped, for ww_fail

  template <typename T>
  void add(const char *name, const std::vector<T> &v) {
    const size_t off = (bytes.size() + WW_PACK_ALIGN - 1) / WW_PACK_ALIGN * WW_PACK_ALIGN, n = v.size() * sizeof(T);
    bytes.resize(off + n, 0);
    if (n) memcpy(bytes.data() + off, v.data(), n);
    table.push_back({name, (uint32_t)sizeof(T), off, n});
  }
  int fail(int code, const char *fmt, ...) __attribute__((format(printf, 3, 4))) {  // (`this` counts as argument 1)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, sizeof err, fmt, ap);
    va_end(ap);
    return code;
  }
};

struct blob_view {
  const uint8_t *base;
  size_t len;
  uint32_t n, kind;
  // the header; a status and pm.err otherwise
  static int open(ww_packed_model &pm, const void *blob, size_t len, blob_view *bv) {
    if (len < 16) return pm.fail(WW_EBLOB, "blob too short");
    uint32_t h[4];
    memcpy(h, blob, sizeof h);
    if (h[0] != 0x42485757u || h[1] != 1u) return pm.fail(WW_EBLOB, "bad blob magic/version");
    *bv = {(const uint8_t *)blob, len, h[3], h[2]};
    if (16 + 32 * (size_t)bv->n > len) return pm.fail(WW_EBLOB, "section table exceeds blob");
    if (bv->kind != WW_KIND_CRNN && bv->kind != WW_KIND_WAVENET) return pm.fail(WW_EBLOB, "unknown model kind %u", bv->kind);
    return WW_OK;
  }
  // the 4-byte words of section `name`, copied out; false: no such section inside the blob (*count: what its entry says)
  template <typename T>
  bool words(const char *name, std::vector<T> &out, uint32_t *count = nullptr) const {
    static_assert(sizeof(T) == 4, "blob sections hold float32 or int32");
    for (uint32_t i = 0; i < n; ++i) {
      const uint8_t *e = base + 16 + 32 * (size_t)i;
      if (strncmp((const char *)e, name, 24) == 0) {
        uint32_t off, cnt;
        memcpy(&off, e + 24, 4);
        memcpy(&cnt, e + 28, 4);
        if ((size_t)off + (size_t)cnt * 4 > len) return false;
        if (count) *count = cnt;
        out.resize(cnt);
        if (cnt) memcpy(out.data(), base + off, (size_t)cnt * 4);
        return true;
      }
    }
    return false;
  }
  int floats(ww_packed_model &pm, const char *name, size_t expect, std::vector<float> &out) const {
    uint32_t cnt = 0;
    if (!words(name, out, &cnt) || (size_t)cnt != expect)
      return pm.fail(WW_EBLOB, "blob section %s missing or has %u elements (expected %zu)", name, cnt, expect);
    return WW_OK;
  }
  // whether the section table names `name` at all (its extent may still lie outside the blob)
  bool has(const char *name) const {
    for (uint32_t i = 0; i < n; ++i)
      if (strncmp((const char *)(base + 16 + 32 * (size_t)i), name, 24) == 0) return true;
    return false;
  }
  // an int32 section of exactly `expect` words
  bool ints(const char *name, size_t expect, std::vector<int32_t> &out) const { return words(name, out) && out.size() == expect; }
};

#define NEED_F(var, name, cnt_expect) \
  std::vector<float> var;             \
  if (int rc_ = bv.floats(pm, name, (size_t)(cnt_expect), var)) return rc_;

inline int pack_filter(ww_packed_model &pm, const blob_view &bv) {
  std::vector<int32_t> meta;
  if (!bv.ints("filter.meta", 2, meta)) return pm.fail(WW_EBLOB, "blob lacks filter.meta");
  const int n_mel = meta[0], n_bins = meta[1];
  if (n_mel < 1 || n_mel > 40 || n_bins != WW_FFT_BINS)
    return pm.fail(WW_EBLOB, "unsupported filter geometry %d x %d (need <= 40 x 257)", n_mel, n_bins);
  NEED_F(cst, "filter.consts", 3);
  NEED_F(w, "filter.w", (size_t)n_mel * n_bins);
  NEED_F(b, "filter.b", n_mel);
  ww_filter_geom &f = pm.filt;
  f.n_mel = n_mel; f.n_bins = n_bins; f.floor_v = cst[0]; f.log_off = cst[1]; f.scale = cst[2];
  // band i covers bins [start[i], start[i] + len[i])
  std::vector<int> start(n_mel), len(n_mel);
  for (int i = 0; i < n_mel; ++i) {
    int lo = -1, hi = -1;
    for (int k = 0; k < n_bins; ++k)
      if (w[(size_t)i * n_bins + k] != 0.0f) {
        if (lo < 0) lo = k;
        hi = k;
      }
    start[i] = lo < 0 ? 0 : lo;
    len[i] = lo < 0 ? 0 : hi - lo + 1;
    f.total_taps += len[i];
    if (len[i] > f.max_len) f.max_len = len[i];
  }
  if (f.max_len > WW_MEL_TAPS)
    return pm.fail(WW_EBLOB, "mel band of %d taps exceeds the kernel limit of %d", f.max_len, WW_MEL_TAPS);
  std::vector<float> wpad((size_t)WW_MEL_TAPS * 64, 0.f);
  for (int i = 0; i < n_mel; ++i)
    for (int k = 0; k < len[i]; ++k) wpad[(size_t)k * 64 + i] = w[(size_t)i * n_bins + start[i] + k];
  std::vector<double> hann(WW_FFT_WINDOW), tw256(512), tw512(512);
  // np.hanning(M) as NumPy evaluates it: 0.5 + 0.5 cos(pi n / (M-1)), n = 1-M, 3-M, ..., M-1 (exactly symmetric)
  for (int n = 0; n < WW_FFT_WINDOW; ++n)
    hann[n] = 0.5 + 0.5 * cos(M_PI * (double)(2 * n - (WW_FFT_WINDOW - 1)) / (double)(WW_FFT_WINDOW - 1));
  for (int k = 0; k < 256; ++k) {
    tw256[2 * k] = cos(-2.0 * M_PI * k / 256.0);
    tw256[2 * k + 1] = sin(-2.0 * M_PI * k / 256.0);
    tw512[2 * k] = cos(-2.0 * M_PI * k / 512.0);
    tw512[2 * k + 1] = sin(-2.0 * M_PI * k / 512.0);
  }
  std::vector<double> tw16(512);
  for (int k1 = 0; k1 < 16; ++k1)
    for (int jj = 0; jj < 16; ++jj) {
      tw16[2 * (k1 * 16 + jj)] = cos(-2.0 * M_PI * (double)(jj * k1) / 256.0);
      tw16[2 * (k1 * 16 + jj) + 1] = sin(-2.0 * M_PI * (double)(jj * k1) / 256.0);
    }
  pm.add("filt.tw16", tw16);
  // mel filter in lane form (frontend.hip, logmel_kernel): bands sorted by width, widest first, dealt to
  // groups of 16 slots with 36 / 16 / 12 padded taps.  Weights carry the 0.5 of the real-FFT untangling
  // (exact), and a band's first bin is pulled back so that its padded taps stay inside the zero-padded
  // row of MAG_LD magnitudes.
  {
    static const int capq[WW_MELV_GROUPS] = WW_MELV_CAPQ, chunk0[WW_MELV_GROUPS] = WW_MELV_CHUNK0;
    const int cap[WW_MELV_GROUPS] = {4 * capq[0], 4 * capq[1], 4 * capq[2]};
    if (n_mel > 16 * WW_MELV_GROUPS)
      return pm.fail(WW_EBLOB, "mel filterbank has %d bands; the lane form holds %d", n_mel, 16 * WW_MELV_GROUPS);
    std::vector<int> order(n_mel);
    for (int i = 0; i < n_mel; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return len[x] > len[y]; });
    // First bins are rounded down to a multiple of 4 when every band still fits its group's taps: the kernel
    // then reads the magnitudes 16 bytes at a time.  A ds_read_b128 is served in four groups of 16 lanes
    // ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32); with lane = 4 slot + frame those hold the
    // slots {0,3,5,6}, {1,2,4,7}, {8,11,13,14}, {9,10,12,15}, and the four frames' rows lie 4 sixteen-byte bank
    // slots apart.  So the four bands of such a quad should start on different bank slots mod 4: where the
    // taps leave room a band's first bin is pulled back further to get there.
    static const int quad[4][4] = {{0, 3, 5, 6}, {1, 2, 4, 7}, {8, 11, 13, 14}, {9, 10, 12, 15}};
    bool aligned = true;
    for (int r = 0; r < n_mel; ++r) {
      const int g = r / 16, band = order[r];
      if (len[band] > cap[g])
        return pm.fail(WW_EBLOB, "mel band %d spans %d bins; the lane form takes %d for the %d widest, %d for the next 16, %d for the rest",
                       band, len[band], cap[0], 16, cap[1], cap[2]);
      int s0 = start[band] < MAG_LD - cap[g] ? start[band] : MAG_LD - cap[g];
      if (start[band] - (s0 & ~3) + len[band] > cap[g]) aligned = false;
    }
    std::vector<float> melV((size_t)WW_MELV_CHUNKS * 16 * 4, 0.f);
    std::vector<int> slots(WW_MELV_GROUPS * 16, 0xffff << 16);
    for (int g = 0; g < WW_MELV_GROUPS; ++g) {
      const int nb = n_mel - 16 * g < 0 ? 0 : (n_mel - 16 * g > 16 ? 16 : n_mel - 16 * g);
      int s0v[16], slotv[16], cls_n[4] = {0, 0, 0, 0};
      // least flexible bands choose their residue class first
      std::vector<int> idx(nb);
      for (int i = 0; i < nb; ++i) idx[i] = i;
      auto room = [&](int i) {  // how many steps of 4 bins band i can be pulled back beyond the plain rounding
        const int band = order[16 * g + i];
        int s0 = start[band] < MAG_LD - cap[g] ? start[band] : MAG_LD - cap[g];
        if (!aligned) return 0;
        s0 &= ~3;
        int n = 0;
        while (s0 - 4 * (n + 1) >= 0 && start[band] - (s0 - 4 * (n + 1)) + len[band] <= cap[g]) ++n;
        return n;
      };
      std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return room(x) < room(y); });
      for (int i : idx) {
        const int band = order[16 * g + i];
        int s0 = start[band] < MAG_LD - cap[g] ? start[band] : MAG_LD - cap[g];
        if (aligned) s0 &= ~3;
        int best = 0, best_n = 1 << 30;
        for (int n = 0; n <= room(i) && n < 4; ++n) {
          const int cls = ((s0 - 4 * n) / 4) & 3;
          if (cls_n[cls] < best_n) { best_n = cls_n[cls]; best = n; }
        }
        s0 -= 4 * best;
        s0v[i] = s0;
        const int cls = (s0 / 4) & 3;
        // class member number q goes to quad q (a fifth member of a class takes any free slot below)
        slotv[i] = cls_n[cls] < 4 ? quad[cls_n[cls]][cls] : -1;
        ++cls_n[cls];
      }
      bool used[16] = {false};
      for (int i = 0; i < nb; ++i)
        if (slotv[i] >= 0) {
          if (used[slotv[i]]) slotv[i] = -1; else used[slotv[i]] = true;
        }
      for (int i = 0; i < nb; ++i)
        if (slotv[i] < 0)
          for (int sl = 0; sl < 16; ++sl)
            if (!used[sl]) { slotv[i] = sl; used[sl] = true; break; }
      for (int i = 0; i < nb; ++i) {
        const int band = order[16 * g + i], slot = slotv[i], s0 = s0v[i];
        for (int k = 0; k < len[band]; ++k) {
          const int t = start[band] - s0 + k;
          melV[((size_t)(chunk0[g] + t / 4) * 16 + slot) * 4 + t % 4] = 0.5f * w[(size_t)band * n_bins + start[band] + k];
        }
        slots[g * 16 + slot] = s0 | (band << 16);
      }
      // empty slots read (zero-weighted) magnitudes too: park each on the bank slot its quad still lacks
      for (int q = 0; q < 4; ++q) {
        bool have[4] = {false, false, false, false};
        for (int c = 0; c < 4; ++c)
          if (used[quad[q][c]]) have[((slots[g * 16 + quad[q][c]] & 0xffff) / 4) & 3] = true;
        for (int c = 0; c < 4; ++c)
          if (!used[quad[q][c]])
            for (int cls = 0; cls < 4; ++cls)
              if (!have[cls]) { have[cls] = true; slots[g * 16 + quad[q][c]] = (4 * cls) | (0xffff << 16); break; }
      }
    }
    f.melv_aligned = aligned ? 1 : 0;
    pm.add("filt.melV", melV);
    pm.add("filt.melVmeta", slots);
  }
  pm.add("filt.start", start); pm.add("filt.bias", b); pm.add("filt.wpad", wpad); pm.add("filt.wdense", w);
  pm.add("filt.hann", hann); pm.add("filt.tw256", tw256); pm.add("filt.tw512", tw512);
  return WW_OK;
}

// split-bf16 mode (WW_PRECISION_BF16X3): x = hi + lo, both bf16 round-to-nearest-even
inline uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf16_f(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
inline void bf16_split(float x, uint16_t &hi, uint16_t &lo) {
  hi = bf16_rne(x);
  lo = bf16_rne(x - bf16_f(hi));
}

// a row-major [n_rows][k] matrix in MFMA B-operand order [k/4][n_rows][4]
inline std::vector<float> pack_k4(const std::vector<float> &src, size_t n_rows, size_t k) {
  std::vector<float> dst(src.size());
  for (size_t n = 0; n < n_rows; ++n)
    for (size_t kk = 0; kk < k; ++kk) dst[((kk / 4) * n_rows + n) * 4 + (kk % 4)] = src[n * k + kk];
  return dst;
}

inline int pack_crnn(ww_packed_model &pm, const blob_view &bv) {
  std::vector<int32_t> meta;
  if (!bv.ints("crnn.meta", 14, meta)) return pm.fail(WW_EBLOB, "blob lacks crnn.meta");
  ww_crnn_geom &c = pm.crnn;
  c.n_mel = meta[0]; c.T = meta[1]; c.C = meta[2]; c.KF = meta[3]; c.KT = meta[4]; c.SF = meta[5]; c.ST = meta[6];
  c.PF = meta[7]; c.PT = meta[8]; c.OF = meta[9]; c.OT = meta[10]; c.H = meta[11]; c.NOUT = meta[12]; c.HEAD = meta[13];
  // Every word is bounded before any arithmetic on it.  A window holds at most 16,384 values (T * n_mel, n_mel >= 1), so no
  // kernel extent, stride, padding or output count of a conv over it can exceed 16,384 either: with these bounds every product
  // below (K = KF * KT, OF * C, (OT - 1) * ST, C * K, ...) stays under 2^31.  It is also conv_generic_kernel's bound: the kernel
  // stages a window in 4 * T * n_mel <= 65,536 bytes of dynamic LDS, the most a launch is given without hipFuncSetAttribute.
  const int LIM = 16384;
  auto in = [](int x, int lo, int hi) { return x >= lo && x <= hi; };
  // the optional crnn.cell = [cell, F] (wwhip/weights.py writes it only for what crnn.meta cannot say): absent, a GRU under a 2H-wide
  // head.  Each word is tested before anything is computed from it - F = 2 * H below only once H is one of four values.
  if (c.H != 16 && c.H != 32 && c.H != 48 && c.H != 64)
    return pm.fail(WW_EBLOB, "unsupported CRNN recurrent width H = %d (the cells are built for 16, 32, 48 and 64 units)", c.H);
  c.CELL = WW_CELL_GRU;
  c.F = 2 * c.H;
  if (bv.has("crnn.cell")) {
    std::vector<int32_t> cell;
    if (!bv.ints("crnn.cell", 2, cell)) return pm.fail(WW_EBLOB, "blob section crnn.cell is not two words [cell, F] inside the blob");
    if (cell[0] != WW_CELL_GRU && cell[0] != WW_CELL_LSTM)
      return pm.fail(WW_EBLOB, "unknown CRNN recurrent cell %d (0 GRU, 1 LSTM)", cell[0]);
    if (!in(cell[1], 1, 64)) return pm.fail(WW_EBLOB, "unsupported CRNN head width F = %d (the head takes 1..64)", cell[1]);
    c.CELL = cell[0];
    c.F = cell[1];
  }
  // (a CTC head has no first layer, so no F of its own: its blob is refused by the CTC rule below, which names the cell it takes)
  if (c.F > 64 && c.HEAD != WW_HEAD_CTC) return pm.fail(WW_EBLOB, "unsupported CRNN head width F = %d (2H without crnn.cell; the head takes 1..64)", c.F);
  if (!in(c.C, 1, 64) || !in(c.NOUT, 1, 8) || c.n_mel != pm.filt.n_mel || !in(c.T, 1, LIM) ||
      (int64_t)c.T * c.n_mel > LIM || !in(c.KF, 1, LIM) || !in(c.KT, 1, LIM) || !in(c.SF, 1, LIM) || !in(c.ST, 1, LIM) ||
      !in(c.OF, 1, LIM) || !in(c.OT, 1, LIM) || !in(c.PF, 0, LIM) || !in(c.PT, 0, LIM))
    return pm.fail(WW_EBLOB, "unsupported CRNN geometry (C=%d H=%d K=%dx%d stride %dx%d)", c.C, c.H, c.KF, c.KT, c.SF, c.ST);
  const int K = c.KF * c.KT;
  // the geometry of wwdetect/CRNN/train.py:27-49 (every current export) runs on the kernels built for it
  const bool std_conv = c.C == 32 && c.n_mel == 40 && c.T == 151 && c.KF == 5 && c.KT == 20 && c.SF == 2 && c.ST == 8 && c.PF == 1 &&
                        c.PT == 6 && c.OF == 20 && c.OT == 19;
  // ... and so does the cell they are built for: a reset-after GRU of 32 units under a 64-wide head
  const bool std_cell = c.CELL == WW_CELL_GRU && c.H == 32 && c.F == 64;
  c.generic = !(std_conv && std_cell);
  c.FEATP = (c.OF * c.C + 63) / 64 * 64;
  c.SEQP = (2 * c.H + 63) / 64 * 64;
  if (!in(c.HEAD, WW_HEAD_SIGMOID, WW_HEAD_CTC)) return pm.fail(WW_EBLOB, "unknown CRNN head kind %d (0 sigmoid, 1 softmax, 2 CTC)", c.HEAD);
  if (c.HEAD == WW_HEAD_CTC) {
    // gru_tail_ctc_kernel (crnn.hip) is built for the 19 steps of the standard geometry and deals its softmax rows to groups of eight
    // lanes; a CTC output needs a label and the blank.  Whatever loads, ww_ctc_* can launch.
    std::vector<float> none;
    if (!(c.CELL == WW_CELL_GRU && c.H == 32))
      return pm.fail(WW_EBLOB, "a CTC head (HEAD = 2) takes a GRU of 32 units only, not cell %d of %d units", c.CELL, c.H);
    if (!std_cell) return pm.fail(WW_EBLOB, "a CTC head (HEAD = 2) has no first dense layer: crnn.cell gives F = %d", c.F);
    if (c.generic) return pm.fail(WW_EBLOB, "a CTC head (HEAD = 2) takes the standard conv geometry only (19 steps of 640 features)");
    if (!in(c.NOUT, 2, 8)) return pm.fail(WW_EBLOB, "a CTC head (HEAD = 2) has 2..8 classes (labels + blank), not %d", c.NOUT);
    if (bv.words("crnn.head_w1", none) || bv.words("crnn.head_b1", none))
      return pm.fail(WW_EBLOB, "a CTC head (HEAD = 2) has one dense layer: the blob carries crnn.head_w1 / crnn.head_b1");
  }
  NEED_F(cw, "crnn.conv_w", (size_t)c.C * K);
  NEED_F(cb, "crnn.conv_b", c.C);
  if (!c.generic) {
    std::vector<float> w4((size_t)CV_KPAD / 4 * 32 * 4, 0.f);
    for (int ch = 0; ch < c.C; ++ch)
      for (int k = 0; k < K; ++k) w4[((size_t)(k / 4) * 32 + ch) * 4 + (k % 4)] = cw[(size_t)ch * K + k];
    pm.add("crnn.conv_w", w4);
    // the positions at a window's edges see its zero padding: the same conv with the taps over the padding cleared
    // (left: frames kt < PT; right: kt >= KT - (KT - PT - 1) = PT + 7), applied to the stream's real rows (crnn_rows_kernel)
    std::vector<float> wl(w4), wr(w4);
    for (int k = 0; k < K; ++k) {
      const int kt = k % c.KT;
      for (int ch = 0; ch < c.C; ++ch) {
        const size_t o = ((size_t)(k / 4) * 32 + ch) * 4 + (k % 4);
        if (kt < c.PT) wl[o] = 0.f;
        if (kt >= c.T - (c.OT - 1) * c.ST + c.PT) wr[o] = 0.f;   // frames past the window's last row: kt >= 151 - 144 + 6 = 13
      }
    }
    pm.add("crnn.conv_wL", wl);
    pm.add("crnn.conv_wR", wr);
  } else {
    std::vector<float> wt((size_t)K * c.C);
    for (int ch = 0; ch < c.C; ++ch)
      for (int k = 0; k < K; ++k) wt[(size_t)k * c.C + ch] = cw[(size_t)ch * K + k];
    pm.add("crnn.conv_wt", wt);  // (ww_model_load: conv_w is this array too)
  }
  pm.add("crnn.conv_b", cb);
  const int G = (c.CELL == WW_CELL_LSTM ? 4 : 3) * c.H;  // gate rows of one direction
  {  // a Keras LSTM has ONE bias (it travels as bx); a reset-after GRU has two
    static const char *const bhs[4] = {"crnn.g1f.bh", "crnn.g1b.bh", "crnn.g2f.bh", "crnn.g2b.bh"};
    for (const char *name : bhs) {
      if (c.CELL == WW_CELL_LSTM && bv.has(name)) return pm.fail(WW_EBLOB, "an LSTM blob carries %s: an LSTM has one bias, bx", name);
      if (c.CELL == WW_CELL_GRU && !bv.has(name)) return pm.fail(WW_EBLOB, "a GRU blob lacks %s: a reset-after GRU has a recurrent bias", name);
    }
  }
  auto cat2 = [&](const char *a, const char *b, size_t each, std::vector<float> &out) -> int {
    std::vector<float> vb;
    if (!bv.words(a, out) || !bv.words(b, vb) || out.size() != each || vb.size() != each)
      return pm.fail(WW_EBLOB, "blob sections %s/%s missing or mis-sized", a, b);
    out.insert(out.end(), vb.begin(), vb.end());
    return WW_OK;
  };
  std::vector<float> v;
  int rc;
  const size_t in1 = (size_t)c.OF * c.C, in2 = 2 * (size_t)c.H;
  // for an LSTM the device block holds a zero bh of the usual size: no kernel argument is ever null
  auto bh2 = [&](const char *a, const char *b, std::vector<float> &out) -> int {
    if (c.CELL == WW_CELL_LSTM) {
      out.assign(2 * (size_t)G, 0.f);
      return WW_OK;
    }
    return cat2(a, b, G, out);
  };
  if ((rc = cat2("crnn.g1f.wx", "crnn.g1b.wx", G * in1, v))) return rc;  // W_x1 [2*G][OF*C], rows: fwd gates then bwd gates
  if (!c.generic) {
    pm.add("crnn.wx1s", pack_k4(v, 2 * G, in1));
    {  // W_x1 [192][640] -> [plane][k-step 20][n-tile 12][lane = g*16 + j][8]: element e is W[nt*16 + j][ks*32 + 8 g + e]
      const size_t plane = (size_t)WX1B_KS * WX1B_NT * 64 * 8;
      std::vector<unsigned short> wb(2 * plane);
      for (int ks = 0; ks < WX1B_KS; ++ks)
        for (int nt = 0; nt < WX1B_NT; ++nt)
          for (int ln = 0; ln < 64; ++ln)
            for (int e = 0; e < 8; ++e) {
              const int gq = ln >> 4, jj = ln & 15;
              uint16_t h, l;
              bf16_split(v[(size_t)(nt * 16 + jj) * in1 + ks * 32 + 8 * gq + e], h, l);
              const size_t o = (((size_t)ks * WX1B_NT + nt) * 64 + ln) * 8 + e;
              wb[o] = h;
              wb[plane + o] = l;
            }
      pm.add("crnn.wx1b", wb);
    }
    {  // conv weights [32][5][20] -> [plane][k-step 4][m-tile 2][lane = g*16 + i][8]: group G = ks*4 + g = kf*3 + h holds
       // kt'' = 8 h + e with kt = kt'' - 2 (zero outside 0..19); G = 15 is all zero
      const size_t plane = (size_t)CWB_KS * CWB_MT * 64 * 8;
      std::vector<unsigned short> wb(2 * plane, 0);
      for (int ks = 0; ks < CWB_KS; ++ks)
        for (int mt = 0; mt < CWB_MT; ++mt)
          for (int ln = 0; ln < 64; ++ln)
            for (int e = 0; e < 8; ++e) {
              const int gq = ln >> 4, ii = ln & 15, Gq = ks * 4 + gq;
              const int kf = Gq / 3, kt = (Gq % 3) * 8 + e - 2;
              float x = 0.f;
              if (Gq < 15 && kt >= 0 && kt < c.KT) x = cw[(size_t)(mt * 16 + ii) * K + kf * c.KT + kt];
              uint16_t h, l;
              bf16_split(x, h, l);
              const size_t o = (((size_t)ks * CWB_MT + mt) * 64 + ln) * 8 + e;
              wb[o] = h;
              wb[plane + o] = l;
            }
      pm.add("crnn.cwb", wb);
    }
  } else {
    std::vector<float> wp((size_t)2 * G * c.FEATP, 0.f);
    for (int r = 0; r < 2 * G; ++r) memcpy(&wp[(size_t)r * c.FEATP], &v[(size_t)r * in1], in1 * sizeof(float));
    pm.add("crnn.wx1p", wp);
  }
  if ((rc = cat2("crnn.g1f.bx", "crnn.g1b.bx", G, v))) return rc; pm.add("crnn.bx1", v);
  if ((rc = cat2("crnn.g1f.wh", "crnn.g1b.wh", (size_t)G * c.H, v))) return rc; pm.add("crnn.wh1", v);
  if ((rc = bh2("crnn.g1f.bh", "crnn.g1b.bh", v))) return rc; pm.add("crnn.bh1", v);
  if ((rc = cat2("crnn.g2f.wx", "crnn.g2b.wx", G * in2, v))) return rc;
  if ((size_t)c.SEQP == in2) {
    pm.add("crnn.wx2", v);
  } else {
    // gemm_nt_kernel walks K in whole blocks of 64: at 2H = 32 or 96 layer 2's operand rows are SEQP wide, zero padded, as wx1p's
    // are FEATP wide (the layer-1 sequence has the same row stride, its pad columns written as zeros by rnn_layer_kernel)
    std::vector<float> wp((size_t)2 * G * c.SEQP, 0.f);
    for (int r = 0; r < 2 * G; ++r) memcpy(&wp[(size_t)r * c.SEQP], &v[(size_t)r * in2], in2 * sizeof(float));
    pm.add("crnn.wx2", wp);
  }
  pm.add("crnn.wx2s", pack_k4(v, 2 * G, in2));
  if ((rc = cat2("crnn.g2f.bx", "crnn.g2b.bx", G, v))) return rc; pm.add("crnn.bx2", v);
  if ((rc = cat2("crnn.g2f.wh", "crnn.g2b.wh", (size_t)G * c.H, v))) return rc; pm.add("crnn.wh2", v);
  if ((rc = bh2("crnn.g2f.bh", "crnn.g2b.bh", v))) return rc; pm.add("crnn.bh2", v);
  // a CTC head has no first layer: its w1 / b1 are zeros of the same size, so that no kernel argument of any form is a null pointer
  // (the launchers refuse a CTC model long before: crnn.hip, ww_crnn_refuse_ctc)
  std::vector<float> w1((size_t)c.F * in2, 0.f), b1((size_t)c.F, 0.f);  // w1 [F][2H]
  if (c.HEAD != WW_HEAD_CTC) {
    if ((rc = bv.floats(pm, "crnn.head_w1", (size_t)c.F * in2, w1)) || (rc = bv.floats(pm, "crnn.head_b1", (size_t)c.F, b1))) return rc;
  }
  NEED_F(w2, "crnn.head_w2", (size_t)c.NOUT * (c.HEAD == WW_HEAD_CTC ? in2 : (size_t)c.F));
  NEED_F(b2, "crnn.head_b2", c.NOUT);
  pm.add("crnn.w1", w1); pm.add("crnn.b1", b1); pm.add("crnn.w2", w2); pm.add("crnn.b2", b2);
  pm.info.window = c.T; pm.info.n_out = c.NOUT; pm.info.enc_width = 2 * c.H;
  pm.info.enc_rows = c.HEAD == WW_HEAD_CTC ? c.OT : 1;  // (a CTC encoder returns the whole sequence)
  return WW_OK;
}

inline int pack_wave(ww_packed_model &pm, const blob_view &bv) {
  std::vector<int32_t> meta;
  if (!bv.ints("wave.meta", 6, meta)) return pm.fail(WW_EBLOB, "blob lacks wave.meta");
  ww_wave_geom &v = pm.wave;
  v.T = meta[0]; v.n_mel = meta[1]; v.C = meta[2]; v.S = meta[3]; v.NB = meta[4]; v.NOUT = meta[5];
  // NB <= 32: the kernels carry a block's dilation in 4 bits of wave_args::dil4[2] and its residual flag in a bit of a 32-bit mask,
  // and size their LDS vector table (WV_VT_F), BatchNorm table and the sequence form's history for 32 blocks (wavenet.hip).
  if (v.C != 16 || v.S != 32 || v.T > 192 || v.T < 1 || v.n_mel > 48 || v.NOUT < 1 || v.NOUT > 16 || v.NB < 1 || v.NB > 32 ||
      v.n_mel != pm.filt.n_mel)
    return pm.fail(WW_EBLOB, "unsupported Wavenet geometry (T=%d C=%d S=%d NB=%d NOUT=%d n_mel=%d)", v.T, v.C, v.S, v.NB, v.NOUT, v.n_mel);
  const int NB = v.NB, C = v.C, S = v.S;
  std::vector<int32_t> dil, order, has_res;
  if (!bv.ints("wave.dilations", NB, dil)) return pm.fail(WW_EBLOB, "blob lacks wave.dilations");
  if (!bv.ints("wave.skip_order", NB, order)) return pm.fail(WW_EBLOB, "blob lacks wave.skip_order");
  if (!bv.ints("wave.has_res", NB, has_res)) return pm.fail(WW_EBLOB, "blob lacks wave.has_res");
  for (int b = 0; b < NB; ++b) {
    if (dil[b] < 1 || dil[b] > 8) return pm.fail(WW_EBLOB, "dilation %d unsupported (max 8)", dil[b]);  // (2 dil <= WV_PAD rows)
    if (order[b] != b) return pm.fail(WW_EBLOB, "skip connections are not summed in block order");
  }
  v.dil.assign(dil.begin(), dil.end()); v.order.assign(order.begin(), order.end()); v.has_res.assign(has_res.begin(), has_res.end());
  NEED_F(w_in, "wave.w_in", (size_t)v.n_mel * C);
  NEED_F(b_in, "wave.b_in", C);
  NEED_F(bn_s, "wave.bn_scale", (size_t)NB * C);
  NEED_F(bn_t, "wave.bn_shift", (size_t)NB * C);
  NEED_F(w_sig, "wave.w_sig", (size_t)NB * 3 * C * C);
  NEED_F(b_sig, "wave.b_sig", (size_t)NB * C);
  NEED_F(w_tanh, "wave.w_tanh", (size_t)NB * 3 * C * C);
  NEED_F(b_tanh, "wave.b_tanh", (size_t)NB * C);
  NEED_F(w_res, "wave.w_res", (size_t)NB * C * C);
  NEED_F(b_res, "wave.b_res", (size_t)NB * C);
  NEED_F(w_skip, "wave.w_skip", (size_t)NB * C * S);
  NEED_F(b_skip, "wave.b_skip", (size_t)NB * S);
  NEED_F(dw1, "wave.det_w1", (size_t)S * S);
  NEED_F(db1, "wave.det_b1", S);
  NEED_F(dw2, "wave.det_w2", (size_t)S * v.NOUT);
  NEED_F(db2, "wave.det_b2", v.NOUT);
  // MFMA B-operand order: [k-block][kk][col][q], k = kb*16 + kk*4 + q
  std::vector<float> in4(3 * 4 * 16 * 4, 0.f);
  for (int k = 0; k < v.n_mel; ++k)
    for (int col = 0; col < C; ++col) in4[(((k / 16) * 4 + (k % 16) / 4) * 16 + col) * 4 + (k % 4)] = w_in[(size_t)k * C + col];
  std::vector<float> g4((size_t)NB * 3 * 4 * 32 * 4), bg((size_t)NB * 32), rs4((size_t)NB * 4 * 48 * 4), brs((size_t)NB * 48);
  for (int b = 0; b < NB; ++b) {
    for (int tap = 0; tap < 3; ++tap)
      for (int ch = 0; ch < C; ++ch)
        for (int col = 0; col < 32; ++col) {
          float val = col < 16 ? w_sig[(((size_t)b * 3 + tap) * C + ch) * C + col]
                               : w_tanh[(((size_t)b * 3 + tap) * C + ch) * C + col - 16];
          g4[((((size_t)b * 3 + tap) * 4 + ch / 4) * 32 + col) * 4 + (ch % 4)] = val;
        }
    for (int col = 0; col < 16; ++col) {
      bg[(size_t)b * 32 + col] = b_sig[(size_t)b * C + col];
      bg[(size_t)b * 32 + 16 + col] = b_tanh[(size_t)b * C + col];
    }
    for (int ch = 0; ch < C; ++ch)
      for (int col = 0; col < 48; ++col) {
        float val = col < 16 ? w_res[((size_t)b * C + ch) * C + col] : w_skip[((size_t)b * C + ch) * S + col - 16];
        rs4[(((size_t)b * 4 + ch / 4) * 48 + col) * 4 + (ch % 4)] = val;
      }
    for (int col = 0; col < 48; ++col) brs[(size_t)b * 48 + col] = col < 16 ? b_res[(size_t)b * C + col] : b_skip[(size_t)b * S + col - 16];
  }
  std::vector<float> d1((size_t)2 * 4 * 32 * 4), d2((size_t)2 * 4 * 16 * 4, 0.f), d2b(16, 0.f);
  for (int k = 0; k < S; ++k) {
    for (int col = 0; col < S; ++col) d1[(((size_t)(k / 16) * 4 + (k % 16) / 4) * 32 + col) * 4 + (k % 4)] = dw1[(size_t)k * S + col];
    for (int col = 0; col < v.NOUT; ++col) d2[(((size_t)(k / 16) * 4 + (k % 16) / 4) * 16 + col) * 4 + (k % 4)] = dw2[(size_t)k * v.NOUT + col];
  }
  for (int col = 0; col < v.NOUT; ++col) d2b[col] = db2[col];
  // split-bf16 A operands (wavenet.hip, SPLIT_BF16; transposed formulation: rows = output channels).
  // slot = (kstep*2 + {sig,tanh})*2 + {0,1} for the gate conv (k-step 0 = tap 2, k-step 1 = tap 0 | tap 1: the two
  // delayed taps), 8 + mtile*2 + {0,1} for res | skip.  Lane (i = lane & 15, kg = lane >> 4) holds 8 k-slots = two
  // groups of the 4 channels 4 kg .. 4 kg + 3 for output row 16 mtile + i.  Where only one tap (or the gate product) is at
  // hand the second group carries the hi x lo product instead of zeros: 5 MFMAs per gate and 2 per res | skip m-tile give
  // all three split products plus the bias (16 MFMAs per block and tile, not 21).
  {
    std::vector<uint16_t> pk((size_t)NB * WV_PAGE_U4 * 8, 0);  // one page per block
    auto put = [&](int b, int slot, int lane, int q, uint16_t val) { pk[((((size_t)b * WV_SLOTS + slot) * 64) + lane) * 8 + q] = val; };
    for (int b = 0; b < NB; ++b) {
      for (int lane = 0; lane < 64; ++lane) {
        const int i = lane & 15, kg = lane >> 4;
        for (int q = 0; q < 8; ++q) {
          const int ch = 4 * kg + (q & 3);
          for (int mt = 0; mt < 2; ++mt) {
            // the gates are evaluated with v_exp_f32 (= exp2): sigmoid(s) = 1 / (1 + exp2(-log2e s)),
            // tanh(t) = 1 - 2 / (1 + exp2(2 log2e t)) - the factors ride in the weights and biases
            const float sc = mt == 0 ? -1.4426950408889634f : 2.8853900817779268f;
            const std::vector<float> &wsrc = mt == 0 ? w_sig : w_tanh;
            auto wt = [&](int tap) { return wsrc[(((size_t)b * 3 + tap) * C + ch) * C + i] * sc; };
            uint16_t hi, lo;
            // k-step 0, slot "hh": (hi of tap 2 | hi of tap 2) against B = (u_hi | u_lo);
            //           slot "lb": (lo of tap 2 | bias hi, bias lo in k-slots 4, 5 of lane group 0) against B = (u_hi | 1, 1, 0, 0)
            bf16_split(wt(2), hi, lo);
            put(b, (0 * 2 + mt) * 2 + 0, lane, q, hi);
            if (q < 4) {
              put(b, (0 * 2 + mt) * 2 + 1, lane, q, lo);
            } else if (kg == 0 && q < 6) {
              uint16_t bh, bl;
              bf16_split((mt == 0 ? b_sig : b_tanh)[(size_t)b * C + i] * sc, bh, bl);
              put(b, (0 * 2 + mt) * 2 + 1, lane, q, q == 4 ? bh : bl);
            }
            // k-step 1: (tap 0 | tap 1), hi and lo slots, against B = the two delayed rows (hi plane, then lo plane)
            bf16_split(wt(q < 4 ? 0 : 1), hi, lo);
            put(b, (1 * 2 + mt) * 2 + 0, lane, q, hi);
            put(b, (1 * 2 + mt) * 2 + 1, lane, q, lo);
          }
          for (int mt = 0; mt < 3; ++mt) {
            // res | skip: slot "hh" = (hi | hi) against B = (g_hi | g_lo), slot "lb" = (lo | bias hi, bias lo) against (g_hi | 1, 1, 0, 0)
            const float wv = mt == 0 ? (has_res[b] ? w_res[((size_t)b * C + ch) * C + i] : 0.f) : w_skip[((size_t)b * C + ch) * S + (mt - 1) * 16 + i];
            uint16_t hi, lo;
            bf16_split(wv, hi, lo);
            put(b, 8 + mt * 2 + 0, lane, q, hi);
            if (q < 4) {
              put(b, 8 + mt * 2 + 1, lane, q, lo);
            } else if (kg == 0 && q < 6) {
              uint16_t bh, bl;
              bf16_split(mt == 0 ? (has_res[b] ? b_res[(size_t)b * C + i] : 0.f) : b_skip[(size_t)b * S + (mt - 1) * 16 + i], bh, bl);
              put(b, 8 + mt * 2 + 1, lane, q, q == 4 ? bh : bl);
            }
          }
        }
      }
    }
    pm.add("wave.wpk", pk);
  }
  pm.add("wave.w_in", in4); pm.add("wave.b_in", b_in); pm.add("wave.bn_s", bn_s); pm.add("wave.bn_t", bn_t);
  pm.add("wave.w_gate", g4); pm.add("wave.b_gate", bg); pm.add("wave.w_rs", rs4); pm.add("wave.b_rs", brs);
  pm.add("wave.d_w1", d1); pm.add("wave.d_b1", db1); pm.add("wave.d_w2", d2); pm.add("wave.d_b2", d2b);
  pm.info.window = v.T; pm.info.n_out = v.NOUT; pm.info.enc_rows = v.T; pm.info.enc_width = S;
  return WW_OK;
}

#undef NEED_F

// blob -> pm; WW_OK, or a status with pm.err set
inline int ww_pack_model(ww_packed_model &pm, const void *blob, size_t len) {
  blob_view bv;
  int rc = blob_view::open(pm, blob, len, &bv);
  if (rc != WW_OK) return rc;
  pm.kind = (int)bv.kind;
  if ((rc = pack_filter(pm, bv)) != WW_OK) return rc;
  if ((rc = bv.kind == WW_KIND_CRNN ? pack_crnn(pm, bv) : pack_wave(pm, bv)) != WW_OK) return rc;
  pm.info.kind = pm.kind;
  pm.info.n_mel = pm.filt.n_mel;
  pm.info.n_bins = pm.filt.n_bins;
  return WW_OK;
}

}  // namespace
