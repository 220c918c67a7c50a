// model_set.h - the host-only half of ww_model_set (include/wwhip.h): what makes K loaded models members of ONE set, the stride of
// their blocks in the set's allocation, the translation of member 0's device pointers into the set's block, and the checks of the
// member ids a call brings.  Plain C++ (no HIP header, no HIP call): csrc/api.hip and csrc/streams.hip include it;
// tests/native/model_set_check.cpp compiles it alone under Address + UB sanitizer on the CPU (tests/test_model_set_host.py).
//
// A model is one device block whose layout is a function of its geometry alone (model_pack.h): K models of one geometry are K
// blocks of one size, copied to [k * stride, k * stride + block_bytes) of the set's allocation.  A kernel takes member 0's
// pointers - translated into the set's block here - and adds member * stride to each (common.h: ww_set_ref).
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/wwhip.h"
#include "model_layout.h"

#define WW_SET_ALIGN 256  // a member's block starts on a multiple of this (model_pack.h: WW_PACK_ALIGN, every array's alignment)

static inline size_t ww_set_stride(size_t block_bytes) { return (block_bytes + WW_SET_ALIGN - 1) / WW_SET_ALIGN * WW_SET_ALIGN; }

// The filter's arrays of a packed model as one byte string: every table entry whose name starts with "filt.", in table order, each
// as {name, NUL, size (8 bytes), bytes}.  Two models share a front end exactly when these strings are equal.
// Entry: model_pack.h's ww_pack_entry (name, off, bytes).
template <typename Entry>
static inline std::vector<uint8_t> ww_set_filter_image(const std::vector<Entry> &table, const uint8_t *bytes) {
  std::vector<uint8_t> img;
  for (const Entry &e : table) {
    if (strncmp(e.name, "filt.", 5) != 0) continue;
    const size_t nl = strlen(e.name) + 1;
    const uint64_t sz = (uint64_t)e.bytes;
    img.insert(img.end(), (const uint8_t *)e.name, (const uint8_t *)e.name + nl);
    img.insert(img.end(), (const uint8_t *)&sz, (const uint8_t *)&sz + sizeof sz);
    img.insert(img.end(), bytes + e.off, bytes + e.off + e.bytes);
  }
  return img;
}

// What the set looks at of one member (api.hip fills it from a ww_model, the test from a ww_packed_model).
struct ww_set_member {
  const void *ctx = nullptr;  // the context the member was loaded on
  int kind = 0, precision = 0;
  ww_model_info info = {};
  const ww_filter_geom *filt = nullptr;
  const ww_crnn_geom *crnn = nullptr;
  const ww_wave_geom *wave = nullptr;
  size_t block_bytes = 0;
  const std::vector<uint8_t> *filt_image = nullptr;
};

static inline int ww_set_refuse(char *err, size_t cap, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
static inline int ww_set_refuse(char *err, size_t cap, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  if (err && cap) vsnprintf(err, cap, fmt, ap);
  va_end(ap);
  return WW_EINVAL;
}

// field-by-field (not memcmp over the structs: their padding is not part of the geometry); floats by their bits
static inline bool ww_set_same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }
static inline bool ww_set_same_info(const ww_model_info &a, const ww_model_info &b) {
  return a.kind == b.kind && a.window == b.window && a.n_mel == b.n_mel && a.n_bins == b.n_bins && a.n_out == b.n_out &&
         a.enc_rows == b.enc_rows && a.enc_width == b.enc_width && a.reserved == b.reserved;
}
static inline bool ww_set_same_filter(const ww_filter_geom &a, const ww_filter_geom &b) {
  return a.n_mel == b.n_mel && a.n_bins == b.n_bins && ww_set_same_bits(a.floor_v, b.floor_v) && ww_set_same_bits(a.log_off, b.log_off) &&
         ww_set_same_bits(a.scale, b.scale) && a.total_taps == b.total_taps && a.max_len == b.max_len && a.melv_aligned == b.melv_aligned;
}
static inline bool ww_set_same_crnn(const ww_crnn_geom &a, const ww_crnn_geom &b) {
  return a.n_mel == b.n_mel && a.T == b.T && a.C == b.C && a.KF == b.KF && a.KT == b.KT && a.SF == b.SF && a.ST == b.ST && a.PF == b.PF &&
         a.PT == b.PT && a.OF == b.OF && a.OT == b.OT && a.H == b.H && a.NOUT == b.NOUT && a.HEAD == b.HEAD && a.generic == b.generic &&
         a.FEATP == b.FEATP && a.CELL == b.CELL && a.F == b.F && a.SEQP == b.SEQP;
}
static inline bool ww_set_same_wave(const ww_wave_geom &a, const ww_wave_geom &b) {
  return a.T == b.T && a.n_mel == b.n_mel && a.C == b.C && a.S == b.S && a.NB == b.NB && a.NOUT == b.NOUT && a.dil == b.dil &&
         a.order == b.order && a.has_res == b.has_res && a.order_is_natural == b.order_is_natural;
}

// May these n models be one set on context `ctx`?  WW_OK, or WW_EINVAL with the reason in err.
static inline int ww_set_check(const ww_set_member *mem, int32_t n, const void *ctx, char *err, size_t cap) {
  if (n < 1 || n > WW_SET_MAX_MODELS) return ww_set_refuse(err, cap, "a model set has 1..%d members, not %d", WW_SET_MAX_MODELS, (int)n);
  if (!mem) return ww_set_refuse(err, cap, "NULL argument");
  for (int k = 0; k < n; ++k) {
    const ww_set_member &m = mem[k], &m0 = mem[0];
    if (!m.filt || !m.crnn || !m.wave || !m.filt_image) return ww_set_refuse(err, cap, "member %d is NULL", k);
    if (m.ctx != ctx) return ww_set_refuse(err, cap, "member %d was loaded on another context", k);
    if (m.kind != WW_KIND_CRNN && m.kind != WW_KIND_WAVENET) return ww_set_refuse(err, cap, "member %d is of unknown kind %d", k, m.kind);
    if (m.precision != WW_PRECISION_FP32)
      return ww_set_refuse(err, cap, "member %d is in split-bf16 mode: model sets are fp32 only", k);
    if (m.kind == WW_KIND_CRNN && m.crnn->generic && !(m.crnn->CELL == WW_CELL_GRU && m.crnn->H == 32 && m.crnn->F == 64))
      return ww_set_refuse(err, cap, "member %d is a CRNN of cell %d (0 GRU, 1 LSTM), %d units and a %d-wide head, which runs the generic layered path: model sets "
                           "take a GRU of 32 units under a 64-wide head at the standard conv geometry only", k, m.crnn->CELL, m.crnn->H, m.crnn->F);
    if (m.kind == WW_KIND_CRNN && m.crnn->generic)
      return ww_set_refuse(err, cap, "member %d is a CRNN of generic conv geometry: model sets take the standard geometry only", k);
    if (m.kind != m0.kind) return ww_set_refuse(err, cap, "member %d is of kind %d, member 0 of kind %d: one set, one kind", k, m.kind, m0.kind);
    if (!ww_set_same_info(m.info, m0.info))
      return ww_set_refuse(err, cap, "member %d's model info differs from member 0's (window %d / %d, n_out %d / %d, encoder %d x %d / %d x %d)", k,
                           m.info.window, m0.info.window, m.info.n_out, m0.info.n_out, m.info.enc_rows, m.info.enc_width, m0.info.enc_rows,
                           m0.info.enc_width);
    if (m.kind == WW_KIND_CRNN ? !ww_set_same_crnn(*m.crnn, *m0.crnn) : !ww_set_same_wave(*m.wave, *m0.wave))
      return ww_set_refuse(err, cap, "member %d's geometry differs from member 0's%s", k,
                           m.kind == WW_KIND_WAVENET ? " (sizes, dilations, block order or residual convs)" : "");
    // (behind the comparison: a member whose head alone differs from member 0's is a geometry mismatch like any other)
    if (m.kind == WW_KIND_CRNN && m.crnn->HEAD == WW_HEAD_CTC)
      return ww_set_refuse(err, cap, "member %d is a CTC-trained CRNN: it runs alone, through ww_ctc_forward and its family, not in a model set", k);
    if (m.block_bytes != m0.block_bytes)
      return ww_set_refuse(err, cap, "member %d's device block has %zu bytes, member 0's %zu", k, m.block_bytes, m0.block_bytes);
    if (!ww_set_same_filter(*m.filt, *m0.filt) || *m.filt_image != *m0.filt_image)
      return ww_set_refuse(err, cap, "member %d's filter differs from member 0's: one front end serves the whole set", k);
  }
  if (mem[0].block_bytes == 0) return ww_set_refuse(err, cap, "member 0 has no device block");
  return WW_OK;
}

// Every member id of a host table lies in [0, n_models): WW_OK, or WW_EINVAL naming the first that does not.  ids == nullptr: all 0.
static inline int ww_set_check_ids(const int32_t *ids, int64_t n, int32_t n_models, const char *what, char *err, size_t cap) {
  if (!ids) return WW_OK;
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= n_models)
      return ww_set_refuse(err, cap, "%s[%lld] = %d: the set has members 0..%d", what, (long long)i, (int)ids[i], (int)n_models - 1);
  return WW_OK;
}

// The address in the set's block of what p addresses in member 0's own block (member 0 is the set's first copy); nullptr stays
// nullptr.  false: p lies outside the member's block - nothing is translated.
template <typename T>
static inline bool ww_set_translate(T *&p, const void *member_block, size_t block_bytes, void *set_block) {
  if (!p) return true;
  const char *lo = (const char *)member_block, *q = (const char *)p;
  if (q < lo || q >= lo + block_bytes) return false;
  p = (T *)((char *)set_block + (q - lo));
  return true;
}

// Every device pointer of the three structs, by reference (f: a generic callable over T *&).  The static_asserts catch a pointer
// that was added to a struct and not here.
template <typename F>
static inline void ww_set_each_pointer(ww_filter_dev &f_, F &&f) {
  f(f_.start); f(f_.bias); f(f_.wdense); f(f_.wpad); f(f_.hann); f(f_.tw256); f(f_.tw512); f(f_.tw16); f(f_.melV); f(f_.melVmeta);
}
template <typename F>
static inline void ww_set_each_pointer(ww_crnn_dev &c, F &&f) {
  f(c.conv_w); f(c.conv_b); f(c.wx1s); f(c.bx1); f(c.wh1); f(c.bh1); f(c.wx2); f(c.wx2s); f(c.cwb); f(c.wx1b); f(c.bx2); f(c.wh2);
  f(c.bh2); f(c.w1); f(c.b1); f(c.w2); f(c.b2); f(c.conv_wt); f(c.conv_wL); f(c.conv_wR); f(c.wx1p);
}
template <typename F>
static inline void ww_set_each_pointer(ww_wave_dev &v, F &&f) {
  f(v.w_in); f(v.b_in); f(v.bn_s); f(v.bn_t); f(v.w_gate); f(v.b_gate); f(v.w_rs); f(v.b_rs); f(v.d_w1); f(v.d_b1); f(v.d_w2); f(v.d_b2);
  f(v.wpk);
}
static_assert(sizeof(ww_filter_dev) == (sizeof(ww_filter_geom) + 7) / 8 * 8 + 10 * sizeof(void *), "ww_set_each_pointer(ww_filter_dev) misses a pointer");
static_assert(sizeof(ww_crnn_dev) == (sizeof(ww_crnn_geom) + 7) / 8 * 8 + 21 * sizeof(void *), "ww_set_each_pointer(ww_crnn_dev) misses a pointer");
static_assert(sizeof(ww_wave_dev) == (sizeof(ww_wave_geom) + 7) / 8 * 8 + 13 * sizeof(void *), "ww_set_each_pointer(ww_wave_dev) misses a pointer");

// The three structs of member 0, translated into the set's block.  false: a pointer lay outside member 0's block.
static inline bool ww_set_translate_model(ww_filter_dev &f, ww_crnn_dev &c, ww_wave_dev &v, const void *member_block, size_t block_bytes,
                                          void *set_block) {
  bool ok = true;
  auto tr = [&](auto *&p) { ok = ww_set_translate(p, member_block, block_bytes, set_block) && ok; };
  ww_set_each_pointer(f, tr);
  ww_set_each_pointer(c, tr);
  ww_set_each_pointer(v, tr);
  return ok;
}
