// C ABI of libwwhip.so: context, model upload, host/device entry points (see include/wwhip.h).
#include "common.h"
#include "ctc_align.h"
#include "ctc_beam.h"
#include "ctc_occupancy.h"
#include "ctc_score.h"
#include "model_pack.h"
#include "model_set.h"

#include <algorithm>
#include <cmath>
#include <mutex>

// message of a failure that has no context to carry it (ww_ctx_create, NULL handles): one buffer per host thread, so that
// two threads creating contexts concurrently each read their own text through ww_last_error(NULL)
static thread_local char g_err[512] = {0};

int ww_fail(ww_ctx *ctx, int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  char *dst = ctx ? ctx->err : g_err;
  vsnprintf(dst, 512, fmt, ap);
  va_end(ap);
  return code;
}

int ww_ensure(ww_ctx *ctx, ww_arena &a, size_t bytes, bool pinned) {
  if (bytes <= a.cap) return WW_OK;
  if (a.ptr) {
    hipStreamSynchronize(ctx->stream);
    if (pinned) hipHostFree(a.ptr); else hipFree(a.ptr);
    a.ptr = nullptr;
    a.cap = 0;
  }
  size_t want = bytes + bytes / 4 + (1 << 20);
  hipError_t e = pinned ? hipHostMalloc(&a.ptr, want, hipHostMallocDefault) : hipMalloc(&a.ptr, want);
  if (e != hipSuccess) {
    a.ptr = nullptr;
    return ww_fail(ctx, WW_ENOMEM, "cannot allocate %zu bytes of %s memory: %s", want, pinned ? "pinned host" : "device",
                   hipGetErrorString(e));
  }
  a.cap = want;
  return WW_OK;
}

int ww_tables::send(ww_ctx *ctx, void *d_block) const {
  if (bytes() == 0) return WW_OK;
  const int slot = (int)(ctx->desc_k++ & 1);
  if (!ctx->desc_ev[slot]) WW_HIP(ctx, hipEventCreateWithFlags(&ctx->desc_ev[slot], hipEventDisableTiming));
  if (ctx->desc_busy[slot]) {
    WW_HIP(ctx, hipEventSynchronize(ctx->desc_ev[slot]));
    ctx->desc_busy[slot] = false;
  }
  if (int rc = ww_ensure(ctx, ctx->desc_pin[slot], bytes(), true)) return rc;
  pack(ctx->desc_pin[slot].ptr);
  WW_HIP(ctx, hipMemcpyAsync(d_block, ctx->desc_pin[slot].ptr, bytes(), hipMemcpyHostToDevice, ctx->stream));
  WW_HIP(ctx, hipEventRecord(ctx->desc_ev[slot], ctx->stream));
  ctx->desc_busy[slot] = true;
  return WW_OK;
}


// Staging of a host-pointer call: the buffers its kernels read and write, carved in call order from one arena, and the bytes'
// way in and out.  A call of more than WW_SMALL_IO_BYTES stages in the device arena (hipMemcpyAsync in, hipMemcpyAsync out, one
// synchronise).  A smaller one is latency-bound, and a copy-engine operation costs more than a few KB are worth: it stages in the
// context's pinned arena, which the kernels read and write over the bus themselves (memcpy in, one synchronise, memcpy out).
// Every address handed out is the one the kernels use; the entry point is the same code in both modes.
#define WW_SMALL_IO_BYTES (256u << 10)
struct ww_staged_io {
  ww_ctx *ctx;
  bool pinned = false, synced = false;
  char *base = nullptr;  // the arena as the kernels address it
  char *host = nullptr;  // pinned mode: the same bytes as the host addresses them
  size_t off = 0;
  int rc = WW_OK;        // the first in() that failed: checked once, before the launch
  explicit ww_staged_io(ww_ctx *c) : ctx(c) {}
  // bytes: the sum of the call's carves (ww_bump::need each); dev_extra: device scratch behind them (scratch())
  int init(size_t bytes, size_t dev_extra = 0, bool may_pin = true) {
    pinned = may_pin && bytes <= WW_SMALL_IO_BYTES;
    if (!pinned) {
      if (int r = ww_ensure(ctx, ctx->dev, bytes + dev_extra, false)) return r;
      base = (char *)ctx->dev.ptr;
      return WW_OK;
    }
    if (int r = ww_ensure(ctx, ctx->pinned, bytes + 1024, true)) return r;
    host = (char *)ctx->pinned.ptr;
    if (hipHostGetDevicePointer((void **)&base, host, 0) != hipSuccess)
      return ww_fail(ctx, WW_EHIP, "pinned arena is not visible to the device");
    return dev_extra ? ww_ensure(ctx, ctx->dev, dev_extra, false) : WW_OK;
  }
  template <typename T>
  T *out(size_t n) {  // a buffer the kernels write
    T *r = (T *)(base + off);
    off += ww_bump::need(n, sizeof(T));
    return r;
  }
  template <typename T>
  T *host_of(T *p) const { return (T *)(host + ((char *)p - base)); }  // pinned mode only
  // a buffer of `room` (n if 0) elements that holds the caller's n; src stays the caller's until finish()
  template <typename T>
  T *in(const T *src, size_t n, size_t room = 0) {
    T *d = out<T>(room ? room : n);
    if (pinned) memcpy(host_of(d), src, n * sizeof(T));
    else if (rc == WW_OK) rc = h2d(d, src, n * sizeof(T));
    return d;
  }
  // the model's scratch stays in device memory: behind the carves there, at the device arena's start in pinned mode
  void *scratch(size_t bytes) { return pinned ? ctx->dev.ptr : out<char>(bytes); }
  int fetch(void *dst, const void *buf, size_t bytes) {  // dst is valid after finish()
    if (!pinned) {
      WW_HIP(ctx, hipMemcpyAsync(dst, buf, bytes, hipMemcpyDeviceToHost, ctx->stream));
      return WW_OK;
    }
    if (int r = finish()) return r;
    memcpy(dst, host_of((const char *)buf), bytes);
    return WW_OK;
  }
  int finish() {  // pinned mode synchronises once: it takes calls that launch once
    if (synced) return WW_OK;
    WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
    synced = pinned;
    return WW_OK;
  }

 private:
  int h2d(void *d, const void *s, size_t bytes) {
    WW_HIP(ctx, hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, ctx->stream));
    return WW_OK;
  }
};

extern "C" {

static_assert(WW_ABI == 4, "ww_version's text carries the ABI number");
const char *ww_version(void) WW_NOTHROW { return "wwhip 0.5 (gfx950; ABI 4: ww_stream_create takes flags, ww_host_stage_i16, ww_uploader_*, ww_stream_timeline, ww_model_set_*)"; }

int ww_runtime_info(int32_t *built_hip_version, int32_t *runtime_version, int32_t *driver_version) {
  WW_GUARD_BEGIN
  if (built_hip_version) *built_hip_version = HIP_VERSION;  // headers the library was compiled against
  int rt = 0, drv = 0;
  const hipError_t e1 = hipRuntimeGetVersion(&rt);
  const hipError_t e2 = hipDriverGetVersion(&drv);  // may fail where no GPU is visible: reported as 0
  if (runtime_version) *runtime_version = e1 == hipSuccess ? rt : 0;
  if (driver_version) *driver_version = e2 == hipSuccess ? drv : 0;
  return e1 == hipSuccess ? WW_OK : WW_EHIP;
  WW_GUARD_END(nullptr)
}

const char *ww_last_error(const ww_ctx *ctx) WW_NOTHROW { return ctx ? ctx->err : g_err; }

int ww_ctx_create(int device, void *external_stream, ww_ctx **out) {
  WW_GUARD_BEGIN
  if (!out) return ww_fail(nullptr, WW_EINVAL, "out is NULL");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ww_fail(nullptr, WW_ENODEVICE, "no HIP device visible");
  if (device < 0 || device >= n) return ww_fail(nullptr, WW_EINVAL, "device %d out of range (0..%d)", device, n - 1);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ww_fail(nullptr, WW_EHIP, "hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return ww_fail(nullptr, WW_ENODEVICE, "device %d is %s; libwwhip.so carries gfx950 code only", device, prop.gcnArchName);
  ww_device_scope dev_scope(device);  // the stream and events below are created on `device`; the caller's current device is restored
  if (!dev_scope.ok()) return ww_fail(nullptr, WW_EHIP, "cannot switch to device %d: %s", device, hipGetErrorString(dev_scope.err));
  ww_ctx *c = new ww_ctx();
  c->device = device;
  if (external_stream) {
    c->stream = (hipStream_t)external_stream;
  } else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
      delete c;
      return ww_fail(nullptr, WW_EHIP, "hipStreamCreate failed");
    }
    c->own_stream = true;
  }
  ww_scoped<ww_ctx, ww_ctx_destroy> own(c);
  hipEventCreate(&c->t0);
  hipEventCreate(&c->t1);
  // kernel attributes are per device: set them for this context's device (a second GPU of the process gets its own)
  if (int rc = ww_k_crnn_init_device(c)) {
    snprintf(g_err, sizeof g_err, "%s", c->err);
    return rc;
  }
  *out = own.release();
  return WW_OK;
  WW_GUARD_END(nullptr)
}

int ww_ctx_destroy(ww_ctx *ctx) {
  WW_GUARD_BEGIN
  if (!ctx) return WW_OK;
  ww_device_scope dev_scope(ctx->device);
  hipStreamSynchronize(ctx->stream);
  for (auto &co : ctx->clip_offs) {
    hipFree(co.d_so);
    hipFree(co.d_fo);
  }
  for (auto &kv : ctx->prof)
    for (auto &p : kv.second.pending) {
      hipEventDestroy(p.first);
      hipEventDestroy(p.second);
    }
  if (ctx->dev.ptr) hipFree(ctx->dev.ptr);
  if (ctx->pinned.ptr) hipHostFree(ctx->pinned.ptr);
  for (int k = 0; k < 2; ++k) {
    if (ctx->desc_pin[k].ptr) hipHostFree(ctx->desc_pin[k].ptr);
    if (ctx->desc_ev[k]) hipEventDestroy(ctx->desc_ev[k]);
  }
  hipEventDestroy(ctx->t0);
  hipEventDestroy(ctx->t1);
  if (ctx->own_stream) hipStreamDestroy(ctx->stream);
  delete ctx;
  return WW_OK;
  WW_GUARD_END(nullptr)
}

int ww_ctx_synchronize(ww_ctx *ctx) {
  WW_GUARD_BEGIN
  if (!ctx) return WW_EINVAL;
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return WW_OK;
  WW_GUARD_END(ctx)
}

void *ww_ctx_stream(ww_ctx *ctx) WW_NOTHROW { return ctx ? (void *)ctx->stream : nullptr; }

int ww_profile_enable(ww_ctx *ctx, int on) {
  WW_GUARD_BEGIN
  if (!ctx) return WW_EINVAL;
  ctx->profiling = on != 0;
  return WW_OK;
  WW_GUARD_END(ctx)
}

int ww_profile_read(ww_ctx *ctx, char *json, size_t cap) {
  WW_GUARD_BEGIN
  if (!ctx || !json || cap < 8) return WW_EINVAL;
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::string s = "{";
  bool first = true;
  for (auto &kv : ctx->prof) {
    for (auto &p : kv.second.pending) {
      float ms = 0.f;
      hipEventElapsedTime(&ms, p.first, p.second);
      kv.second.total_ms += ms;
      hipEventDestroy(p.first);
      hipEventDestroy(p.second);
    }
    kv.second.pending.clear();
    char buf[256];
    snprintf(buf, sizeof buf, "%s\"%s\": {\"calls\": %d, \"total_ms\": %.6f}", first ? "" : ", ", kv.first.c_str(),
             kv.second.calls, kv.second.total_ms);
    s += buf;
    first = false;
  }
  s += "}";
  ctx->prof.clear();
  if (s.size() + 1 > cap) return ww_fail(ctx, WW_EINVAL, "profile buffer too small (%zu needed)", s.size() + 1);
  memcpy(json, s.c_str(), s.size() + 1);
  return WW_OK;
  WW_GUARD_END(ctx)
}

int ww_timer_start(ww_ctx *ctx) {
  WW_GUARD_BEGIN
  if (!ctx) return WW_EINVAL;
  WW_HIP(ctx, hipEventRecord(ctx->t0, ctx->stream));
  return WW_OK;
  WW_GUARD_END(ctx)
}

int ww_timer_stop(ww_ctx *ctx, float *ms) {
  WW_GUARD_BEGIN
  if (!ctx || !ms) return WW_EINVAL;
  WW_HIP(ctx, hipEventRecord(ctx->t1, ctx->stream));
  WW_HIP(ctx, hipEventSynchronize(ctx->t1));
  WW_HIP(ctx, hipEventElapsedTime(ms, ctx->t0, ctx->t1));
  return WW_OK;
  WW_GUARD_END(ctx)
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// model load: parsed and packed on the host (model_pack.h), then one device block, one copy
// ------------------------------------------------------------------------------------------
// Where the device address of each packed array goes: the packer's name of an array is "<struct>.<member>" of ww_model.
struct model_slot {
  const char *name;
  void (*set)(ww_model &, void *);
};
#define WW_SLOT(s_, member_) {#s_ "." #member_, [](ww_model &m, void *p) { m.s_.member_ = (decltype(m.s_.member_))p; }}
static const model_slot MODEL_SLOTS[] = {
    WW_SLOT(filt, tw16), WW_SLOT(filt, melV), WW_SLOT(filt, melVmeta), WW_SLOT(filt, start), WW_SLOT(filt, bias), WW_SLOT(filt, wpad),
    WW_SLOT(filt, wdense), WW_SLOT(filt, hann), WW_SLOT(filt, tw256), WW_SLOT(filt, tw512),
    WW_SLOT(crnn, conv_w), WW_SLOT(crnn, conv_wL), WW_SLOT(crnn, conv_wR), WW_SLOT(crnn, conv_wt), WW_SLOT(crnn, conv_b),
    WW_SLOT(crnn, wx1s), WW_SLOT(crnn, wx1b), WW_SLOT(crnn, cwb), WW_SLOT(crnn, wx1p), WW_SLOT(crnn, bx1), WW_SLOT(crnn, wh1),
    WW_SLOT(crnn, bh1), WW_SLOT(crnn, wx2), WW_SLOT(crnn, wx2s), WW_SLOT(crnn, bx2), WW_SLOT(crnn, wh2), WW_SLOT(crnn, bh2),
    WW_SLOT(crnn, w1), WW_SLOT(crnn, b1), WW_SLOT(crnn, w2), WW_SLOT(crnn, b2),
    WW_SLOT(wave, wpk), WW_SLOT(wave, w_in), WW_SLOT(wave, b_in), WW_SLOT(wave, bn_s), WW_SLOT(wave, bn_t), WW_SLOT(wave, w_gate),
    WW_SLOT(wave, b_gate), WW_SLOT(wave, w_rs), WW_SLOT(wave, b_rs), WW_SLOT(wave, d_w1), WW_SLOT(wave, d_b1), WW_SLOT(wave, d_w2),
    WW_SLOT(wave, d_b2),
};
#undef WW_SLOT

extern "C" {

int ww_model_load(ww_ctx *ctx, const void *blob, size_t len, ww_model **out) {
  WW_GUARD_BEGIN
  if (!ctx || !blob || !out) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  *out = nullptr;
  ww_packed_model pm;
  const int rc = ww_pack_model(pm, blob, len);  // (reads the blob through memcpy: the caller's buffer need not be 4-byte aligned)
  if (rc != WW_OK) return ww_fail(ctx, rc, "%s", pm.err);
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  ww_model *m = new ww_model();
  ww_scoped<ww_model, ww_model_free> own(m);
  m->ctx = ctx;
  m->kind = pm.kind;
  m->info = pm.info;
  static_cast<ww_filter_geom &>(m->filt) = pm.filt;
  static_cast<ww_crnn_geom &>(m->crnn) = pm.crnn;
  static_cast<ww_wave_geom &>(m->wave) = pm.wave;
  if (hipMalloc(&m->block, pm.bytes.size()) != hipSuccess ||
      hipMemcpy(m->block, pm.bytes.data(), pm.bytes.size(), hipMemcpyHostToDevice) != hipSuccess)
    return ww_fail(ctx, WW_ENOMEM, "model upload failed (%zu bytes)", pm.bytes.size());  // (`own` frees the block)
  for (const ww_pack_entry &e : pm.table) {
    const model_slot *slot = std::find_if(std::begin(MODEL_SLOTS), std::end(MODEL_SLOTS), [&](const model_slot &s) { return strcmp(s.name, e.name) == 0; });
    if (slot == std::end(MODEL_SLOTS)) return ww_fail(ctx, WW_EINTERNAL, "packed array %s has no place in ww_model", e.name);
    slot->set(*m, (char *)m->block + e.off);
  }
  if (m->kind == WW_KIND_CRNN && m->crnn.generic) m->crnn.conv_w = m->crnn.conv_wt;  // one array, the generic kernels' name for it
  m->block_bytes = pm.bytes.size();
  m->filt_image = ww_set_filter_image(pm.table, pm.bytes.data());  // (what ww_model_set_create compares)
  *out = own.release();
  return WW_OK;
  WW_GUARD_END(ctx)
}

int ww_model_free(ww_model *m) {
  WW_GUARD_BEGIN
  if (!m) return WW_OK;
  if (m->ctx) {
    ww_device_scope dev_scope(m->ctx->device);
    hipStreamSynchronize(m->ctx->stream);
  }
  if (m->block) hipFree(m->block);
  delete m;
  return WW_OK;
  WW_GUARD_END(nullptr)
}

int ww_model_get_info(const ww_model *m, ww_model_info *out) {
  WW_GUARD_BEGIN
  if (!m || !out) return WW_EINVAL;
  *out = m->info;
  return WW_OK;
  WW_GUARD_END(m ? m->ctx : nullptr)
}

int ww_model_head_kind(const ww_model *m, int32_t *out) {
  WW_GUARD_BEGIN
  if (!m || !out) return WW_EINVAL;
  *out = m->kind == WW_KIND_CRNN ? m->crnn.HEAD : WW_HEAD_SOFTMAX;
  return WW_OK;
  WW_GUARD_END(m ? m->ctx : nullptr)
}

int ww_model_rnn_kind(const ww_model *m, int32_t *cell, int32_t *units, int32_t *head_units) {
  WW_GUARD_BEGIN
  if (!m || !cell || !units || !head_units) return WW_EINVAL;
  if (m->kind != WW_KIND_CRNN) return ww_fail(m->ctx, WW_EINVAL, "ww_model_rnn_kind: the model is not a CRNN");
  *cell = m->crnn.CELL;
  *units = m->crnn.H;
  *head_units = m->crnn.F;
  return WW_OK;
  WW_GUARD_END(m ? m->ctx : nullptr)
}

int ww_model_set_precision(ww_model *m, int precision) {
  WW_GUARD_BEGIN
  if (!m) return WW_EINVAL;
  if (precision != WW_PRECISION_FP32 && precision != WW_PRECISION_BF16X3)
    return ww_fail(m->ctx, WW_EINVAL, "unknown precision %d", precision);
  m->precision = precision;
  return WW_OK;
  WW_GUARD_END(m ? m->ctx : nullptr)
}

int ww_model_set_option(ww_model *m, int key, int64_t value) {
  WW_GUARD_BEGIN
  if (!m) return WW_EINVAL;
  if (value < 0 || value > 0x7fffffff) return ww_fail(m->ctx, WW_EINVAL, "option value %lld out of range", (long long)value);
  switch (key) {
    case WW_OPT_CRNN_SPLIT_AT: m->opt_split_at = (int)value; return WW_OK;
    case WW_OPT_CRNN_SLIDE_MIN: m->opt_slide_min = (int)value; return WW_OK;
    case WW_OPT_CRNN_TAIL_MFMA:
      if (value > 2) return ww_fail(m->ctx, WW_EINVAL, "WW_OPT_CRNN_TAIL_MFMA takes 0 (never), 1 (from 9,216 windows per launch) or 2 (always)");
      m->opt_tail_mfma = (int)value;
      return WW_OK;
    case WW_OPT_WAVENET_ROWMAJOR: m->opt_wave_rowmajor = value != 0; return WW_OK;
    case WW_OPT_WAVE_SEQ_SEGMENT: m->opt_wave_seq_segment = (int)value; return WW_OK;
    default: return ww_fail(m->ctx, WW_EINVAL, "unknown model option %d", key);
  }
  WW_GUARD_END(m ? m->ctx : nullptr)
}

// ---- model sets (the host half - what may be one set, the stride, the pointer translation - is model_set.h) ----------------------
int ww_model_set_destroy(ww_model_set *set) {
  WW_GUARD_BEGIN
  if (!set) return WW_OK;
  if (set->ctx) {
    ww_device_scope dev_scope(set->ctx->device);
    hipStreamSynchronize(set->ctx->stream);
    if (set->block) hipFree(set->block);
  }
  delete set;
  return WW_OK;
  WW_GUARD_END(nullptr)
}

int ww_model_set_create(ww_ctx *ctx, const ww_model *const *models, int32_t n_models, ww_model_set **out) {
  WW_GUARD_BEGIN
  if (!ctx || !models || !out) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  *out = nullptr;
  if (n_models < 1 || n_models > WW_SET_MAX_MODELS)
    return ww_fail(ctx, WW_EINVAL, "a model set has 1..%d members, not %d", WW_SET_MAX_MODELS, (int)n_models);
  std::vector<ww_set_member> mem((size_t)n_models);
  for (int k = 0; k < n_models; ++k) {
    const ww_model *m = models[k];
    if (!m) return ww_fail(ctx, WW_EINVAL, "member %d is NULL", k);
    mem[k].ctx = m->ctx; mem[k].kind = m->kind; mem[k].precision = m->precision; mem[k].info = m->info;
    mem[k].filt = &m->filt; mem[k].crnn = &m->crnn; mem[k].wave = &m->wave;
    mem[k].block_bytes = m->block_bytes; mem[k].filt_image = &m->filt_image;
  }
  char why[384];
  if (int rc = ww_set_check(mem.data(), n_models, ctx, why, sizeof why)) return ww_fail(ctx, rc, "ww_model_set_create: %s", why);
  WW_ON_DEVICE(ctx, dev_scope);
  ww_model_set *set = new ww_model_set();
  ww_scoped<ww_model_set, ww_model_set_destroy> own(set);
  set->ctx = ctx;
  set->n = n_models;
  const size_t bytes = models[0]->block_bytes;
  set->stride = ww_set_stride(bytes);
  if (hipMalloc(&set->block, set->stride * (size_t)n_models) != hipSuccess)
    return ww_fail(ctx, WW_ENOMEM, "cannot allocate a set of %d models (%zu bytes)", (int)n_models, set->stride * (size_t)n_models);
  for (int k = 0; k < n_models; ++k)
    WW_HIP(ctx, hipMemcpyAsync((char *)set->block + (size_t)k * set->stride, models[k]->block, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the members may be freed as soon as the call returns
  // member 0 as the launchers see it: its geometry, its pointers inside the set's block; the dispatch options are the library's
  // defaults, whatever member 0's are (ww_set_option moves the two that decide the sliding form)
  set->view = *models[0];
  set->view.block = set->block;
  {
    const ww_model defaults;
    set->view.opt_split_at = defaults.opt_split_at; set->view.opt_slide_min = defaults.opt_slide_min;
    set->view.opt_tail_mfma = defaults.opt_tail_mfma; set->view.opt_wave_rowmajor = defaults.opt_wave_rowmajor;
    set->view.opt_wave_seq_segment = defaults.opt_wave_seq_segment;
  }
  set->view.filt_image.clear();  // (compared above; the view needs no copy of it)
  set->view.filt_image.shrink_to_fit();
  if (!ww_set_translate_model(set->view.filt, set->view.crnn, set->view.wave, models[0]->block, bytes, set->block))
    return ww_fail(ctx, WW_EINTERNAL, "ww_model_set_create: a pointer of member 0 lies outside its block");
  *out = own.release();
  return WW_OK;
  WW_GUARD_END(ctx)
}

// The two options that decide the sliding form's launches and the segment length of the sequence form (the view starts from the
// library's defaults)
int ww_set_option(ww_model_set *set, int key, int64_t value) {
  WW_GUARD_BEGIN
  if (!set) return WW_EINVAL;
  if (value < 0 || value > 0x7fffffff) return ww_fail(set->ctx, WW_EINVAL, "option value %lld out of range", (long long)value);
  switch (key) {
    case WW_OPT_CRNN_SLIDE_MIN: set->view.opt_slide_min = (int)value; return WW_OK;
    case WW_OPT_CRNN_TAIL_MFMA:
      if (value > 2) return ww_fail(set->ctx, WW_EINVAL, "WW_OPT_CRNN_TAIL_MFMA takes 0 (never), 1 (from 9,216 windows per launch) or 2 (always)");
      set->view.opt_tail_mfma = (int)value;
      return WW_OK;
    case WW_OPT_WAVE_SEQ_SEGMENT: set->view.opt_wave_seq_segment = (int)value; return WW_OK;
    default:
      return ww_fail(set->ctx, WW_EINVAL, "a model set takes WW_OPT_CRNN_SLIDE_MIN, WW_OPT_CRNN_TAIL_MFMA and WW_OPT_WAVE_SEQ_SEGMENT, not option %d", key);
  }
  WW_GUARD_END(set ? set->ctx : nullptr)
}

int ww_model_set_info(const ww_model_set *set, ww_model_info *info, int32_t *n_models) {
  WW_GUARD_BEGIN
  if (!set) return WW_EINVAL;
  if (info) *info = set->view.info;
  if (n_models) *n_models = set->n;
  return WW_OK;
  WW_GUARD_END(set ? set->ctx : nullptr)
}

int64_t ww_num_frames(int64_t n, int32_t hop) WW_NOTHROW {
  if (hop <= 0 || n < WW_FFT_WINDOW) return 0;
  return (n - WW_FFT_WINDOW) / hop + 1;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// front end entry points
// ------------------------------------------------------------------------------------------
static int check_fp(ww_ctx *ctx, const ww_frontend_params *fp, bool need_div) {
  if (!fp) return ww_fail(ctx, WW_EINVAL, "frontend params are NULL");
  if (fp->hop <= 0 || fp->hop > WW_FFT_WINDOW) return ww_fail(ctx, WW_EINVAL, "hop %d out of range (1..512)", fp->hop);
  if (need_div && !(fp->pcm_divisor > 0.f)) return ww_fail(ctx, WW_EINVAL, "pcm_divisor must be positive");
  return WW_OK;
}

static int logmel_host(ww_ctx *ctx, const ww_model *m, const void *samples, size_t elt, const int64_t *sample_offs, int n_utt,
                       const ww_frontend_params *fp, float *mel, int64_t *frame_offs) {
  if (!ctx || !m || !sample_offs || !frame_offs) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (n_utt < 0) return ww_fail(ctx, WW_EINVAL, "negative utterance count");
  int rc = check_fp(ctx, fp, elt == 2);
  if (rc) return rc;
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  frame_offs[0] = 0;
  int64_t max_f = 0;
  for (int u = 0; u < n_utt; ++u) {
    const int64_t n = sample_offs[u + 1] - sample_offs[u];
    if (n < 0) return ww_fail(ctx, WW_EINVAL, "sample_offs not ascending at %d", u);
    const int64_t nf = ww_num_frames(n, fp->hop);
    frame_offs[u + 1] = frame_offs[u] + nf;
    if (nf > max_f) max_f = nf;
  }
  const int64_t total_f = frame_offs[n_utt];
  if (n_utt == 0 || total_f == 0) return WW_OK;
  if (!samples || !mel) return ww_fail(ctx, WW_EINVAL, "NULL sample or mel buffer");
  const int64_t base = sample_offs[0], total_s = sample_offs[n_utt] - base;
  const size_t b_s = ww_bump::need((size_t)total_s + 16, elt), b_o = ww_bump::need((size_t)n_utt + 1, 8);
  const size_t b_m = ww_bump::need((size_t)total_f * m->filt.n_mel, 4);
  ww_staged_io io(ctx);
  if ((rc = io.init(b_s + 2 * b_o + b_m))) return rc;
  // the samples, with room for 16 elements of zero padding behind them (zeroed where that is a host memset)
  char *d_s = io.in((const char *)samples + (size_t)base * elt, (size_t)total_s * elt, ((size_t)total_s + 16) * elt);
  if (io.pinned) memset(io.host_of(d_s) + (size_t)total_s * elt, 0, 16 * elt);
  // sample_offs rebased to the first sample staged: written in place in pinned mode, copied from `so` (alive until finish()) otherwise
  std::vector<int64_t> so;
  int64_t *d_so;
  if (io.pinned) {
    int64_t *h_so = io.host_of(d_so = io.out<int64_t>(n_utt + 1));
    for (int u = 0; u <= n_utt; ++u) h_so[u] = sample_offs[u] - base;
  } else {
    so.resize(n_utt + 1);
    for (int u = 0; u <= n_utt; ++u) so[u] = sample_offs[u] - base;
    d_so = io.in(so.data(), n_utt + 1);
  }
  int64_t *d_fo = io.in(frame_offs, n_utt + 1);
  float *d_mel = io.out<float>((size_t)total_f * m->filt.n_mel);
  if (io.rc) return io.rc;
  rc = ww_k_logmel(ctx, m, elt == 2 ? (const int16_t *)d_s : nullptr, elt == 4 ? (const float *)d_s : nullptr, d_so, d_fo,
                   n_utt, total_f, max_f, fp, d_mel, 0, total_s);
  if (rc) return rc;
  if ((rc = io.fetch(mel, d_mel, (size_t)total_f * m->filt.n_mel * 4))) return rc;
  return io.finish();
}

extern "C" {

int ww_logmel(ww_ctx *ctx, const ww_model *m, const int16_t *pcm, const int64_t *sample_offs, int32_t n_utt,
              const ww_frontend_params *fp, float *mel, int64_t *frame_offs) {
  WW_GUARD_BEGIN
  return logmel_host(ctx, m, pcm, 2, sample_offs, n_utt, fp, mel, frame_offs);
  WW_GUARD_END(ctx)
}

int ww_logmel_f32(ww_ctx *ctx, const ww_model *m, const float *samples, const int64_t *sample_offs, int32_t n_utt,
                  const ww_frontend_params *fp, float *mel, int64_t *frame_offs) {
  WW_GUARD_BEGIN
  return logmel_host(ctx, m, samples, 4, sample_offs, n_utt, fp, mel, frame_offs);
  WW_GUARD_END(ctx)
}

int ww_logmel_dev(ww_ctx *ctx, const ww_model *m, const int16_t *d_pcm, const int64_t *d_sample_offs,
                  const int64_t *d_frame_offs, int32_t n_utt, int64_t total_frames, int64_t max_frames_per_utt,
                  const ww_frontend_params *fp, float *d_mel) {
  WW_GUARD_BEGIN
  if (!ctx || !m || !d_pcm || !d_sample_offs || !d_frame_offs || !d_mel) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (((uintptr_t)d_pcm & 15) != 0) return ww_fail(ctx, WW_EINVAL, "d_pcm must be 16-byte aligned");
  int rc = check_fp(ctx, fp, true);
  if (rc) return rc;
  WW_ON_DEVICE(ctx, dev);
  return ww_k_logmel(ctx, m, d_pcm, nullptr, d_sample_offs, d_frame_offs, n_utt, total_frames, max_frames_per_utt, fp, d_mel);
  WW_GUARD_END(ctx)
}

int ww_stft_mag(ww_ctx *ctx, const ww_model *m, const float *frames, int64_t n, int32_t precise, float *mag) {
  WW_GUARD_BEGIN
  if (!ctx || !m) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative frame count");
  if (n == 0) return WW_OK;
  if (!frames || !mag) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  const size_t b_f = ww_bump::need((size_t)n * WW_FFT_WINDOW, 4), b_m = ww_bump::need((size_t)n * WW_FFT_BINS, 4);
  ww_staged_io io(ctx);
  int rc = io.init(b_f + b_m);
  if (rc) return rc;
  const float *d_f = io.in(frames, (size_t)n * WW_FFT_WINDOW);
  float *d_m = io.out<float>((size_t)n * WW_FFT_BINS);
  if (io.rc) return io.rc;
  if ((rc = ww_k_stft_mag(ctx, m, d_f, n, precise, d_m))) return rc;
  if ((rc = io.fetch(mag, d_m, (size_t)n * WW_FFT_BINS * 4))) return rc;
  return io.finish();
  WW_GUARD_END(ctx)
}

}  // extern "C"

extern "C" {

int ww_filter_apply(ww_ctx *ctx, const ww_model *m, const float *mag, int64_t n, float *mel) {
  WW_GUARD_BEGIN
  if (!ctx || !m) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative row count");
  if (n == 0) return WW_OK;
  if (!mag || !mel) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  const int NBN = m->filt.n_bins, F = m->filt.n_mel;
  const size_t b_a = ww_bump::need((size_t)n * NBN, 4), b_b = ww_bump::need((size_t)n * F, 4);
  ww_staged_io io(ctx);
  int rc = io.init(b_a + b_b);
  if (rc) return rc;
  const float *d_a = io.in(mag, (size_t)n * NBN);
  float *d_b = io.out<float>((size_t)n * F);
  if (io.rc) return io.rc;
  if ((rc = ww_k_mel_only(ctx, m, d_a, n, d_b))) return rc;
  if ((rc = io.fetch(mel, d_b, (size_t)n * F * 4))) return rc;
  return io.finish();
  WW_GUARD_END(ctx)
}

int ww_detect(ww_ctx *ctx, const ww_model *m, const float *enc, int32_t n, float *out) {
  WW_GUARD_BEGIN
  if (!ctx || !m) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (int rc_ctc = ww_crnn_refuse_ctc(ctx, m, "ww_detect")) return rc_ctc;
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative row count");
  if (n == 0) return WW_OK;
  if (!enc || !out) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  const size_t per = (size_t)m->info.enc_rows * m->info.enc_width;
  const size_t b_a = ww_bump::need((size_t)n * per, 4), b_b = ww_bump::need((size_t)n * m->info.n_out, 4);
  ww_staged_io io(ctx);
  int rc = io.init(b_a + b_b);
  if (rc) return rc;
  const float *d_a = io.in(enc, (size_t)n * per);
  float *d_b = io.out<float>((size_t)n * m->info.n_out);
  if (io.rc) return io.rc;
  rc = m->kind == WW_KIND_CRNN ? ww_k_crnn_detect(ctx, m, d_a, n, d_b) : ww_k_wave_detect(ctx, m, d_a, n, d_b);
  if (rc) return rc;
  if ((rc = io.fetch(out, d_b, (size_t)n * m->info.n_out * 4))) return rc;
  return io.finish();
  WW_GUARD_END(ctx)
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// encode + detect entry points
// ------------------------------------------------------------------------------------------
static size_t model_ws(const ww_model *m, int nw) {
  return m->kind == WW_KIND_CRNN ? ww_crnn_workspace(m, nw) : ww_wave_workspace(m, nw);
}

// ws: model scratch inside the context's device arena (ww_ensure'd by the caller for model_ws(m, nw) or more): its capacity is
// what is left of the arena behind it.  set: a model set's explicit windows (m: the set's view, window w by member set->ids[w])
static int model_forward(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_row,
                         const int32_t *d_valid, int64_t row0, int hop, int valid_const, int nw, void *ws, float *d_out,
                         float *d_enc, const ww_set_ref *set = nullptr) {
  const char *lo = (const char *)ctx->dev.ptr, *p = (const char *)ws;
  const size_t cap = (p >= lo && p <= lo + ctx->dev.cap) ? (size_t)(lo + ctx->dev.cap - p) : 0;
  return m->kind == WW_KIND_CRNN
             ? ww_k_crnn_forward(ctx, m, d_mel, mel_rows, d_row, d_valid, row0, hop, valid_const, nw, ws, cap, d_out, d_enc, nullptr, set)
             : ww_k_wave_forward(ctx, m, d_mel, mel_rows, d_row, d_valid, row0, hop, valid_const, nw, ws, cap, d_out, d_enc, nullptr, set);
}

// windows are processed in chunks so that the workspace stays bounded
#ifndef WW_MAX_CHUNK
#define WW_MAX_CHUNK 16384
#endif

static int chunk_of(int64_t nw) { return nw < WW_MAX_CHUNK ? (int)nw : WW_MAX_CHUNK; }

// model_forward over nw windows, chunk_of(nw) at a time, ws sized for one chunk.  The windows slide over the mel rows (d_row ==
// nullptr: window w starts at row w * hop and has valid_const rows) or are an explicit list (d_row, d_valid).  d_out moves on with
// the windows; d_enc holds one chunk's encoder rows, which after_chunk(w0, n) takes away before the next chunk overwrites them.
template <typename AfterChunk>
static int forward_chunks(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_row,
                          const int32_t *d_valid, int hop, int valid_const, int64_t nw, void *ws, float *d_out, float *d_enc,
                          AfterChunk after_chunk) {
  const int chunk = chunk_of(nw), NO = m->info.n_out;
  for (int64_t w0 = 0; w0 < nw; w0 += chunk) {
    const int n = (int)((nw - w0) < chunk ? (nw - w0) : chunk);
    int rc = model_forward(ctx, m, d_mel, mel_rows, d_row ? d_row + w0 : nullptr, d_row ? d_valid + w0 : nullptr, d_row ? 0 : w0 * hop,
                           hop, valid_const, n, ws, d_out + (size_t)w0 * NO, d_enc);
    if (rc || (rc = after_chunk(w0, n))) return rc;
  }
  return WW_OK;
}
static int no_enc(int64_t, int) { return WW_OK; }  // the after_chunk of a caller that asks for no encoder rows

// The reference's per-frame use (one window in, one posterior out, utils/time_tf_models.py) is the staging's pinned mode: no
// host-to-device or device-to-host copy on its path.  Pinned mode synchronises once, so it is for calls of one chunk.
static int forward_host(ww_ctx *ctx, const ww_model *m, const float *mel, int64_t rows, int hop, int64_t nw, float *out,
                        float *enc) {
  const int T = m->info.window, F = m->info.n_mel, NO = m->info.n_out, chunk = chunk_of(nw);
  const size_t enc_per = (size_t)m->info.enc_rows * m->info.enc_width;
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  const size_t b_mel = ww_bump::need((size_t)rows * F, 4), b_out = ww_bump::need((size_t)nw * NO, 4);
  const size_t b_enc = enc ? ww_bump::need((size_t)chunk * enc_per, 4) : 0;
  const size_t b_ws = model_ws(m, chunk);
  ww_staged_io io(ctx);
  int rc = io.init(b_mel + b_out + b_enc, b_ws + 1024, nw <= 64 && nw <= WW_MAX_CHUNK);
  if (rc) return rc;
  const float *d_mel = io.in(mel, (size_t)rows * F);
  float *d_out = io.out<float>((size_t)nw * NO);
  float *d_enc = enc ? io.out<float>((size_t)chunk * enc_per) : nullptr;
  void *ws = io.scratch(b_ws);
  if (io.rc) return io.rc;
  rc = forward_chunks(ctx, m, d_mel, rows, nullptr, nullptr, hop, T, nw, ws, d_out, d_enc, [&](int64_t w0, int n) -> int {
    if (!enc) return WW_OK;
    if (int r = io.fetch(enc + (size_t)w0 * enc_per, d_enc, (size_t)n * enc_per * 4)) return r;
    return io.finish();
  });
  if (rc) return rc;
  if ((rc = io.fetch(out, d_out, (size_t)nw * NO * 4))) return rc;
  return io.finish();
}

// ---- CTC-trained CRNNs (include/wwhip.h: ww_ctc_*) ------------------------------------------------------------------------------
#define WW_CTC_STEPS 19  // the standard geometry's conv positions: a CTC model loads at no other (model_pack.h)

// what the three model entry points of the family refuse, before anything is written
static int ctc_check(ww_ctx *ctx, const ww_model *m, int32_t max_labels, const void *labels, const void *lengths, const char *what) {
  if (!ctx || !m) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (int rc = ww_crnn_ctc_check(ctx, m, what)) return rc;
  if (max_labels < 1 || max_labels > WW_CTC_STEPS) return ww_fail(ctx, WW_EINVAL, "%s: max_labels %d outside 1..%d", what, (int)max_labels, WW_CTC_STEPS);
  if (!labels || !lengths) return ww_fail(ctx, WW_EINVAL, "%s: labels / lengths are NULL", what);
  return WW_OK;
}

// ww_k_crnn_ctc_forward over nw windows, chunk_of(nw) at a time, as forward_chunks: sliding windows (d_row == nullptr) or an explicit
// list; every output moves on with the windows.  ws: scratch inside the context's device arena, sized for one chunk.
static int ctc_chunks(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_row, const int32_t *d_valid,
                      int hop, int valid_const, int64_t nw, void *ws, int max_labels, int32_t *d_labels, int32_t *d_lengths, float *d_steps,
                      float *d_enc) {
  const char *lo = (const char *)ctx->dev.ptr, *p = (const char *)ws;
  const size_t cap = (p >= lo && p <= lo + ctx->dev.cap) ? (size_t)(lo + ctx->dev.cap - p) : 0;
  const int chunk = chunk_of(nw), L = m->info.n_out;
  const size_t per_enc = (size_t)m->info.enc_rows * m->info.enc_width;
  for (int64_t w0 = 0; w0 < nw; w0 += chunk) {
    const int n = (int)((nw - w0) < chunk ? (nw - w0) : chunk);
    if (int rc = ww_k_crnn_ctc_forward(ctx, m, d_mel, mel_rows, d_row ? d_row + w0 : nullptr, d_row ? d_valid + w0 : nullptr, d_row ? 0 : w0 * hop,
                                       hop, valid_const, n, ws, cap, max_labels, d_labels + (size_t)w0 * max_labels, d_lengths + w0,
                                       d_steps ? d_steps + (size_t)w0 * WW_CTC_STEPS * L : nullptr, d_enc ? d_enc + (size_t)w0 * per_enc : nullptr))
      return rc;
  }
  return WW_OK;
}

// the host forms: the sequence in, every output the caller asked for out, staged like forward_host's
static int ctc_host(ww_ctx *ctx, const ww_model *m, const float *mel, int64_t rows, int hop, int64_t nw, int max_labels, int32_t *labels,
                    int32_t *lengths, float *steps, float *enc) {
  const int T = m->info.window, F = m->info.n_mel, L = m->info.n_out;
  const size_t per_enc = (size_t)m->info.enc_rows * m->info.enc_width, n_lab = (size_t)nw * max_labels, n_steps = (size_t)nw * WW_CTC_STEPS * L;
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  const size_t b_io = ww_bump::need((size_t)rows * F, 4) + ww_bump::need(n_lab, 4) + ww_bump::need((size_t)nw, 4) +
                      (steps ? ww_bump::need(n_steps, 4) : 0) + (enc ? ww_bump::need((size_t)nw * per_enc, 4) : 0);
  const size_t b_ws = ww_crnn_ctc_workspace(m, chunk_of(nw));
  ww_staged_io io(ctx);
  int rc = io.init(b_io, b_ws + 1024, nw <= 64);
  if (rc) return rc;
  const float *d_mel = io.in(mel, (size_t)rows * F);
  int32_t *d_lab = io.out<int32_t>(n_lab), *d_len = io.out<int32_t>((size_t)nw);
  float *d_steps = steps ? io.out<float>(n_steps) : nullptr, *d_enc = enc ? io.out<float>((size_t)nw * per_enc) : nullptr;
  void *ws = io.scratch(b_ws);
  if (io.rc) return io.rc;
  if ((rc = ctc_chunks(ctx, m, d_mel, rows, nullptr, nullptr, hop, T, nw, ws, max_labels, d_lab, d_len, d_steps, d_enc))) return rc;
  if ((rc = io.fetch(labels, d_lab, n_lab * 4)) || (rc = io.fetch(lengths, d_len, (size_t)nw * 4))) return rc;
  if (steps && (rc = io.fetch(steps, d_steps, n_steps * 4))) return rc;
  if (enc && (rc = io.fetch(enc, d_enc, (size_t)nw * per_enc * 4))) return rc;
  return io.finish();
}

// ---- the forward-algorithm score (include/wwhip.h: ww_ctc_score_*; csrc/ctc_score.h) --------------------------------------------
// the arguments every form shares -> the kernel's argument; WW_EINVAL naming the rule
static int ctc_score_targets_of(ww_ctx *ctx, int T, int L, const int32_t *targets, const int32_t *target_lens, int K, int mode, const char *what,
                                ww_ctc_score_targets &tg) {
  char why[200];
  if (!ww_ctc_score_args_ok(T, L, targets, target_lens, K, mode, why, sizeof why)) return ww_fail(ctx, WW_EINVAL, "%s: %s", what, why);
  memset(&tg, 0, sizeof tg);
  tg.K = K;
  tg.mode = mode;
  for (int k = 0; k < K; ++k) {
    tg.len[k] = (int8_t)target_lens[k];
    for (int u = 0; u < target_lens[k]; ++u) tg.c[k][u] = (int8_t)targets[k * WW_CTC_SCORE_MAX_TARGET + u];
  }
  return WW_OK;
}

// what the three model forms refuse before anything is written: ctc_check's rules (labels and lengths are optional here, together)
static int ctc_score_check(ww_ctx *ctx, const ww_model *m, const int32_t *targets, const int32_t *target_lens, int K, int mode, const void *score,
                           int max_labels, const void *labels, const void *lengths, const char *what, ww_ctc_score_targets &tg) {
  if (!ctx || !m) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (int rc = ww_crnn_ctc_check(ctx, m, what)) return rc;
  if (int rc = ctc_score_targets_of(ctx, WW_CTC_STEPS, m->info.n_out, targets, target_lens, K, mode, what, tg)) return rc;
  if ((labels == nullptr) != (lengths == nullptr)) return ww_fail(ctx, WW_EINVAL, "%s: labels and lengths go together", what);
  if (labels && (max_labels < 1 || max_labels > WW_CTC_STEPS)) return ww_fail(ctx, WW_EINVAL, "%s: max_labels %d outside 1..%d", what, max_labels, WW_CTC_STEPS);
  if (!score) return ww_fail(ctx, WW_EINVAL, "%s: score is NULL", what);
  return WW_OK;
}

// device scratch of ctc_score_chunks for nw windows: a chunk's posteriors, its decode where the caller did not ask for one, the model's
static size_t ctc_score_workspace(const ww_model *m, int64_t nw) {
  const size_t chunk = (size_t)chunk_of(nw);
  return ww_bump::need(chunk * WW_CTC_STEPS * m->info.n_out, 4) + 2 * ww_bump::need(chunk, 4) + ww_crnn_ctc_workspace(m, (int)chunk);
}

// ctc_chunks with the posteriors kept in the workspace and ctc_score_kernel behind every chunk's model launch: d_score [K][nw]
// (d_labels / d_lengths: nullptr, or the decode beside the score; d_score may be nullptr where d_value / d_span are given).  ws: ctc_score_workspace(m, nw) bytes inside the device arena.
static int ctc_score_chunks(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_row, const int32_t *d_valid,
                            int hop, int valid_const, int64_t nw, void *ws, const ww_ctc_score_targets &tg, float *d_score, int max_labels,
                            int32_t *d_labels, int32_t *d_lengths, float *d_value = nullptr, int8_t *d_span = nullptr) {
  const int chunk = chunk_of(nw), L = m->info.n_out;
  ww_bump bump(ws, ctc_score_workspace(m, nw));
  float *d_steps = bump.take<float>((size_t)chunk * WW_CTC_STEPS * L);
  int32_t *own_lab = bump.take<int32_t>((size_t)chunk), *own_len = bump.take<int32_t>((size_t)chunk);
  void *mws = bump.base + bump.off;
  const char *lo = (const char *)ctx->dev.ptr, *p = (const char *)mws;
  const size_t cap = (p >= lo && p <= lo + ctx->dev.cap) ? (size_t)(lo + ctx->dev.cap - p) : 0;
  for (int64_t w0 = 0; w0 < nw; w0 += chunk) {
    const int n = (int)((nw - w0) < chunk ? (nw - w0) : chunk);
    if (int rc = ww_k_crnn_ctc_forward(ctx, m, d_mel, mel_rows, d_row ? d_row + w0 : nullptr, d_row ? d_valid + w0 : nullptr, d_row ? 0 : w0 * hop,
                                       hop, valid_const, n, mws, cap, d_labels ? max_labels : 1, d_labels ? d_labels + (size_t)w0 * max_labels : own_lab,
                                       d_labels ? d_lengths + w0 : own_len, d_steps, nullptr))
      return rc;
    if (d_score)
      if (int rc = ww_k_ctc_score(ctx, d_steps, n, WW_CTC_STEPS, L, tg, d_score + w0, nw, 1)) return rc;
    // the align forms (ww_ctc_align_*): ctc_align_kernel in the score kernel's place, d_value [K][nw] and d_span [K][nw][9][2]
    if (d_value)
      if (int rc = ww_k_ctc_align(ctx, d_steps, n, WW_CTC_STEPS, L, tg, d_value + w0, d_span + w0 * (2 * WW_CTC_SCORE_MAX_TARGET), nw, 1)) return rc;
  }
  return WW_OK;
}

// the host forms: the sequence in, the K planes (and the decode, where asked for) out, staged like ctc_host's
// (score, or value and span: the score forms and the align forms)
static int ctc_score_host(ww_ctx *ctx, const ww_model *m, const float *mel, int64_t rows, int hop, int64_t nw, const ww_ctc_score_targets &tg,
                          float *score, int max_labels, int32_t *labels, int32_t *lengths, float *value = nullptr, int8_t *span = nullptr) {
  const int T = m->info.window, F = m->info.n_mel;
  const size_t n_score = (size_t)nw * tg.K, n_lab = labels ? (size_t)nw * max_labels : 0;
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  const size_t n_span = value ? n_score * 2 * WW_CTC_SCORE_MAX_TARGET : 0;
  const size_t b_io = ww_bump::need((size_t)rows * F, 4) + ww_bump::need(n_score, 4) + ww_bump::need(n_span, 1) + (labels ? ww_bump::need(n_lab, 4) + ww_bump::need((size_t)nw, 4) : 0);
  const size_t b_ws = ctc_score_workspace(m, nw);
  ww_staged_io io(ctx);
  int rc = io.init(b_io, b_ws + 1024, nw <= 64);
  if (rc) return rc;
  const float *d_mel = io.in(mel, (size_t)rows * F);
  float *d_score = io.out<float>(n_score);  // (the align forms: the values)
  int8_t *d_span = value ? io.out<int8_t>(n_span) : nullptr;
  int32_t *d_lab = labels ? io.out<int32_t>(n_lab) : nullptr, *d_len = labels ? io.out<int32_t>((size_t)nw) : nullptr;
  void *ws = io.scratch(b_ws);
  if (io.rc) return io.rc;
  if ((rc = ctc_score_chunks(ctx, m, d_mel, rows, nullptr, nullptr, hop, T, nw, ws, tg, value ? nullptr : d_score, max_labels, d_lab, d_len,
                             value ? d_score : nullptr, d_span)))
    return rc;
  if ((rc = io.fetch(value ? value : score, d_score, n_score * 4))) return rc;
  if (value && (rc = io.fetch(span, d_span, n_span))) return rc;
  if (labels && ((rc = io.fetch(labels, d_lab, n_lab * 4)) || (rc = io.fetch(lengths, d_len, (size_t)nw * 4)))) return rc;
  return io.finish();
}

// ---- the prefix beam search (include/wwhip.h: ww_ctc_beam_*; csrc/ctc_beam.h) --------------------------------------------------------
// what the three model forms refuse before anything is written
static int ctc_beam_check(ww_ctx *ctx, const ww_model *m, int W, int P, int max_labels, const void *labels, const void *lengths, const void *prob,
                          const char *what) {
  if (!ctx || !m) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (int rc = ww_crnn_ctc_check(ctx, m, what)) return rc;
  char why[200];
  if (!ww_ctc_beam_args_ok(WW_CTC_STEPS, m->info.n_out, W, P, max_labels, why, sizeof why)) return ww_fail(ctx, WW_EINVAL, "%s: %s", what, why);
  if (!labels || !lengths || !prob) return ww_fail(ctx, WW_EINVAL, "%s: labels / lengths / prob are NULL", what);
  return WW_OK;
}

// ctc_score_chunks with ctc_beam_kernel behind every chunk's model launch: d_labels [nw][P][max_labels], d_lengths [nw][P], d_prob [nw][P]
// (the greedy decode the model launch also makes stays in the workspace).  ws: ctc_score_workspace(m, nw) bytes inside the device arena.
static int ctc_beam_chunks(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_row, const int32_t *d_valid,
                           int hop, int valid_const, int64_t nw, void *ws, int W, int P, int max_labels, int32_t *d_labels, int32_t *d_lengths,
                           float *d_prob) {
  const int chunk = chunk_of(nw), L = m->info.n_out;
  ww_bump bump(ws, ctc_score_workspace(m, nw));
  float *d_steps = bump.take<float>((size_t)chunk * WW_CTC_STEPS * L);
  int32_t *own_lab = bump.take<int32_t>((size_t)chunk), *own_len = bump.take<int32_t>((size_t)chunk);
  void *mws = bump.base + bump.off;
  const char *lo = (const char *)ctx->dev.ptr, *p = (const char *)mws;
  const size_t cap = (p >= lo && p <= lo + ctx->dev.cap) ? (size_t)(lo + ctx->dev.cap - p) : 0;
  for (int64_t w0 = 0; w0 < nw; w0 += chunk) {
    const int n = (int)((nw - w0) < chunk ? (nw - w0) : chunk);
    if (int rc = ww_k_crnn_ctc_forward(ctx, m, d_mel, mel_rows, d_row ? d_row + w0 : nullptr, d_row ? d_valid + w0 : nullptr, d_row ? 0 : w0 * hop,
                                       hop, valid_const, n, mws, cap, 1, own_lab, own_len, d_steps, nullptr))
      return rc;
    if (int rc = ww_k_ctc_beam(ctx, d_steps, n, WW_CTC_STEPS, L, W, P, max_labels, d_labels + (size_t)w0 * P * max_labels, d_lengths + (size_t)w0 * P,
                               d_prob + (size_t)w0 * P))
      return rc;
  }
  return WW_OK;
}

// the host forms: the sequence in, the P paths of every window out, staged like ctc_score_host's
static int ctc_beam_host(ww_ctx *ctx, const ww_model *m, const float *mel, int64_t rows, int hop, int64_t nw, int W, int P, int max_labels,
                         int32_t *labels, int32_t *lengths, float *prob) {
  const int T = m->info.window, F = m->info.n_mel;
  const size_t n_path = (size_t)nw * P, n_lab = n_path * max_labels;
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  const size_t b_io = ww_bump::need((size_t)rows * F, 4) + ww_bump::need(n_lab, 4) + 2 * ww_bump::need(n_path, 4);
  const size_t b_ws = ctc_score_workspace(m, nw);
  ww_staged_io io(ctx);
  int rc = io.init(b_io, b_ws + 1024, nw <= 64);
  if (rc) return rc;
  const float *d_mel = io.in(mel, (size_t)rows * F);
  int32_t *d_lab = io.out<int32_t>(n_lab), *d_len = io.out<int32_t>(n_path);
  float *d_prob = io.out<float>(n_path);
  void *ws = io.scratch(b_ws);
  if (io.rc) return io.rc;
  if ((rc = ctc_beam_chunks(ctx, m, d_mel, rows, nullptr, nullptr, hop, T, nw, ws, W, P, max_labels, d_lab, d_len, d_prob))) return rc;
  if ((rc = io.fetch(labels, d_lab, n_lab * 4)) || (rc = io.fetch(lengths, d_len, n_path * 4)) || (rc = io.fetch(prob, d_prob, n_path * 4))) return rc;
  return io.finish();
}

// ---- the forward-backward occupancy (include/wwhip.h: ww_ctc_occupancy_*; csrc/ctc_occupancy.h) ---------------------------------------
// what the three model forms refuse before anything is written: the score forms' rules, the occupancy's own (a NULL value or occ, a
// cls in prefix mode)
static int ctc_occupancy_check(ww_ctx *ctx, const ww_model *m, const int32_t *targets, const int32_t *target_lens, int K, int mode, const void *value,
                               const void *occ, const void *cls, int max_labels, const void *labels, const void *lengths, const char *what,
                               ww_ctc_score_targets &tg) {
  if (!ctx || !m) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (int rc = ww_crnn_ctc_check(ctx, m, what)) return rc;
  char why[200];
  if (!ww_ctc_occupancy_args_ok(WW_CTC_STEPS, m->info.n_out, targets, target_lens, K, mode, value, occ, cls, why, sizeof why))
    return ww_fail(ctx, WW_EINVAL, "%s: %s", what, why);
  if ((labels == nullptr) != (lengths == nullptr)) return ww_fail(ctx, WW_EINVAL, "%s: labels and lengths go together", what);
  if (labels && (max_labels < 1 || max_labels > WW_CTC_STEPS)) return ww_fail(ctx, WW_EINVAL, "%s: max_labels %d outside 1..%d", what, max_labels, WW_CTC_STEPS);
  return ctc_score_targets_of(ctx, WW_CTC_STEPS, m->info.n_out, targets, target_lens, K, mode, what, tg);
}

// ctc_score_chunks with ctc_occupancy_kernel behind every chunk's model launch: d_value [K][nw], d_occ [K][nw][19][9] and, where not
// nullptr, d_cls [K][nw][19][L] (d_labels / d_lengths: nullptr, or the decode beside them).  ws: ctc_score_workspace(m, nw) bytes
// inside the device arena.
static int ctc_occupancy_chunks(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_row, const int32_t *d_valid,
                                int hop, int valid_const, int64_t nw, void *ws, const ww_ctc_score_targets &tg, float *d_value, float *d_occ,
                                float *d_cls, int max_labels, int32_t *d_labels, int32_t *d_lengths) {
  const int chunk = chunk_of(nw), L = m->info.n_out;
  ww_bump bump(ws, ctc_score_workspace(m, nw));
  float *d_steps = bump.take<float>((size_t)chunk * WW_CTC_STEPS * L);
  int32_t *own_lab = bump.take<int32_t>((size_t)chunk), *own_len = bump.take<int32_t>((size_t)chunk);
  void *mws = bump.base + bump.off;
  const char *lo = (const char *)ctx->dev.ptr, *p = (const char *)mws;
  const size_t cap = (p >= lo && p <= lo + ctx->dev.cap) ? (size_t)(lo + ctx->dev.cap - p) : 0;
  for (int64_t w0 = 0; w0 < nw; w0 += chunk) {
    const int n = (int)((nw - w0) < chunk ? (nw - w0) : chunk);
    if (int rc = ww_k_crnn_ctc_forward(ctx, m, d_mel, mel_rows, d_row ? d_row + w0 : nullptr, d_row ? d_valid + w0 : nullptr, d_row ? 0 : w0 * hop,
                                       hop, valid_const, n, mws, cap, d_labels ? max_labels : 1, d_labels ? d_labels + (size_t)w0 * max_labels : own_lab,
                                       d_labels ? d_lengths + w0 : own_len, d_steps, nullptr))
      return rc;
    if (int rc = ww_k_ctc_occupancy(ctx, d_steps, n, WW_CTC_STEPS, L, tg, d_value + w0, d_occ + (size_t)w0 * WW_CTC_STEPS * WW_CTC_SCORE_MAX_TARGET,
                                    d_cls ? d_cls + (size_t)w0 * WW_CTC_STEPS * L : nullptr, nw, 1))
      return rc;
  }
  return WW_OK;
}

// the host forms: the sequence in, the K planes of value, occ and (where asked for) cls and the decode out, staged like ctc_score_host's
static int ctc_occupancy_host(ww_ctx *ctx, const ww_model *m, const float *mel, int64_t rows, int hop, int64_t nw, const ww_ctc_score_targets &tg,
                              float *value, float *occ, float *cls, int max_labels, int32_t *labels, int32_t *lengths) {
  const int T = m->info.window, F = m->info.n_mel, L = m->info.n_out;
  const size_t n_val = (size_t)nw * tg.K, n_occ = n_val * WW_CTC_STEPS * WW_CTC_SCORE_MAX_TARGET, n_cls = cls ? n_val * WW_CTC_STEPS * L : 0;
  const size_t n_lab = labels ? (size_t)nw * max_labels : 0;
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  const size_t b_io = ww_bump::need((size_t)rows * F, 4) + ww_bump::need(n_val, 4) + ww_bump::need(n_occ, 4) + (cls ? ww_bump::need(n_cls, 4) : 0) +
                      (labels ? ww_bump::need(n_lab, 4) + ww_bump::need((size_t)nw, 4) : 0);
  const size_t b_ws = ctc_score_workspace(m, nw);
  ww_staged_io io(ctx);
  int rc = io.init(b_io, b_ws + 1024, nw <= 64);
  if (rc) return rc;
  const float *d_mel = io.in(mel, (size_t)rows * F);
  float *d_value = io.out<float>(n_val), *d_occ = io.out<float>(n_occ), *d_cls = cls ? io.out<float>(n_cls) : nullptr;
  int32_t *d_lab = labels ? io.out<int32_t>(n_lab) : nullptr, *d_len = labels ? io.out<int32_t>((size_t)nw) : nullptr;
  void *ws = io.scratch(b_ws);
  if (io.rc) return io.rc;
  if ((rc = ctc_occupancy_chunks(ctx, m, d_mel, rows, nullptr, nullptr, hop, T, nw, ws, tg, d_value, d_occ, d_cls, max_labels, d_lab, d_len))) return rc;
  if ((rc = io.fetch(value, d_value, n_val * 4)) || (rc = io.fetch(occ, d_occ, n_occ * 4))) return rc;
  if (cls && (rc = io.fetch(cls, d_cls, n_cls * 4))) return rc;
  if (labels && ((rc = io.fetch(labels, d_lab, n_lab * 4)) || (rc = io.fetch(lengths, d_len, (size_t)nw * 4)))) return rc;
  return io.finish();
}

__global__ void iota_offs_kernel(int64_t *sample_offs, int64_t *frame_offs, int n, int64_t samples, int64_t frames) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) {
    sample_offs[i] = (int64_t)i * samples;
    frame_offs[i] = (int64_t)i * frames;
  }
}

extern "C" {

int ww_forward_enc(ww_ctx *ctx, const ww_model *m, const float *windows, int32_t nw, float *out, float *enc) {
  WW_GUARD_BEGIN
  if (!ctx || !m) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (int rc_ctc = ww_crnn_refuse_ctc(ctx, m, "ww_forward")) return rc_ctc;
  if (nw < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (nw == 0) return WW_OK;
  if (!windows || !out) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  // B stacked windows are one mel sequence of B*T rows read with hop = T
  return forward_host(ctx, m, windows, (int64_t)nw * m->info.window, m->info.window, nw, out, enc);
  WW_GUARD_END(ctx)
}

int ww_forward(ww_ctx *ctx, const ww_model *m, const float *windows, int32_t nw, float *out) {
  WW_GUARD_BEGIN
  return ww_forward_enc(ctx, m, windows, nw, out, nullptr);
  WW_GUARD_END(ctx)
}

int ww_slide_forward(ww_ctx *ctx, const ww_model *m, const float *mel, int64_t rows, int32_t hop, float *out,
                     int64_t *n_windows) {
  WW_GUARD_BEGIN
  if (!ctx || !m || !n_windows) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (int rc_ctc = ww_crnn_refuse_ctc(ctx, m, "ww_slide_forward")) return rc_ctc;
  if (hop <= 0) return ww_fail(ctx, WW_EINVAL, "hop must be positive");
  if (rows < 0) return ww_fail(ctx, WW_EINVAL, "negative row count");
  const int T = m->info.window;
  const int64_t nw = rows >= T ? (rows - T) / hop + 1 : 0;
  *n_windows = nw;
  if (nw == 0) return WW_OK;
  if (!mel || !out) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  return forward_host(ctx, m, mel, rows, hop, nw, out, nullptr);
  WW_GUARD_END(ctx)
}

int ww_forward_windows_dev(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                           const int32_t *d_win_valid, int32_t nw, float *d_out) {
  WW_GUARD_BEGIN
  if (!ctx || !m || !d_mel || !d_out) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (int rc_ctc = ww_crnn_refuse_ctc(ctx, m, "ww_forward_windows_dev")) return rc_ctc;
  if (nw < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (nw == 0) return WW_OK;
  if (!d_win_row || !d_win_valid) return ww_fail(ctx, WW_EINVAL, "window descriptors are NULL");
  WW_ON_DEVICE(ctx, dev);
  int rc = ww_ensure(ctx, ctx->dev, model_ws(m, chunk_of(nw)) + 1024, false);
  if (rc) return rc;
  return forward_chunks(ctx, m, d_mel, mel_rows, d_win_row, d_win_valid, 0, 0, nw, ctx->dev.ptr, d_out, nullptr, no_enc);
  WW_GUARD_END(ctx)
}

int ww_ctc_forward(ww_ctx *ctx, const ww_model *m, const float *windows, int32_t n, int32_t max_labels, int32_t *labels, int32_t *lengths,
                   float *steps, float *enc) {
  WW_GUARD_BEGIN
  if (int rc = ctc_check(ctx, m, max_labels, labels, lengths, "ww_ctc_forward")) return rc;
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (n == 0) return WW_OK;
  if (!windows) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  // n stacked windows are one mel sequence of n * T rows read with hop = T
  return ctc_host(ctx, m, windows, (int64_t)n * m->info.window, m->info.window, n, max_labels, labels, lengths, steps, enc);
  WW_GUARD_END(ctx)
}

int ww_ctc_slide_forward(ww_ctx *ctx, const ww_model *m, const float *mel, int64_t rows, int32_t hop, int32_t max_labels, int32_t *labels,
                         int32_t *lengths, float *steps, int64_t *n_windows) {
  WW_GUARD_BEGIN
  if (int rc = ctc_check(ctx, m, max_labels, labels, lengths, "ww_ctc_slide_forward")) return rc;
  if (!n_windows) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (hop <= 0) return ww_fail(ctx, WW_EINVAL, "hop must be positive");
  if (rows < 0) return ww_fail(ctx, WW_EINVAL, "negative row count");
  const int T = m->info.window;
  const int64_t nw = rows >= T ? (rows - T) / hop + 1 : 0;
  if (nw > 0 && !mel) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  *n_windows = nw;
  if (nw == 0) return WW_OK;
  return ctc_host(ctx, m, mel, rows, hop, nw, max_labels, labels, lengths, steps, nullptr);
  WW_GUARD_END(ctx)
}

int ww_ctc_forward_windows_dev(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                               const int32_t *d_win_valid, int32_t n, int32_t max_labels, int32_t *d_labels, int32_t *d_lengths,
                               float *d_steps, float *d_enc) {
  WW_GUARD_BEGIN
  if (int rc = ctc_check(ctx, m, max_labels, d_labels, d_lengths, "ww_ctc_forward_windows_dev")) return rc;
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (n == 0) return WW_OK;
  if (!d_mel) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (!d_win_row || !d_win_valid) return ww_fail(ctx, WW_EINVAL, "window descriptors are NULL");
  WW_ON_DEVICE(ctx, dev);
  if (int rc = ww_ensure(ctx, ctx->dev, ww_crnn_ctc_workspace(m, chunk_of(n)) + 1024, false)) return rc;
  return ctc_chunks(ctx, m, d_mel, mel_rows, d_win_row, d_win_valid, 0, 0, n, ctx->dev.ptr, max_labels, d_labels, d_lengths, d_steps, d_enc);
  WW_GUARD_END(ctx)
}

int ww_ctc_greedy_dev(ww_ctx *ctx, const float *d_steps, int64_t n, int32_t T, int32_t L, int32_t max_labels, int32_t *d_labels,
                      int32_t *d_lengths) {
  WW_GUARD_BEGIN
  if (!ctx) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (T < 1 || T > 4096 || L < 2 || L > 64) return ww_fail(ctx, WW_EINVAL, "ww_ctc_greedy_dev: T = %d (1..4096), L = %d (2..64)", (int)T, (int)L);
  if (max_labels < 1 || max_labels > T) return ww_fail(ctx, WW_EINVAL, "ww_ctc_greedy_dev: max_labels %d outside 1..%d", (int)max_labels, (int)T);
  if (n < 0 || n > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "ww_ctc_greedy_dev: sequence count out of range");
  if (n == 0) return WW_OK;
  if (!d_steps || !d_labels || !d_lengths) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  WW_ON_DEVICE(ctx, dev);
  return ww_k_ctc_greedy(ctx, d_steps, n, T, L, max_labels, d_labels, d_lengths);
  WW_GUARD_END(ctx)
}

int ww_ctc_score_dev(ww_ctx *ctx, const float *d_steps, int64_t n, int32_t T, int32_t L, const int32_t *targets, const int32_t *target_lens,
                     int32_t K, int32_t mode, float *d_score) {
  WW_GUARD_BEGIN
  if (!ctx) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  ww_ctc_score_targets tg;
  if (int rc = ctc_score_targets_of(ctx, T, L, targets, target_lens, K, mode, "ww_ctc_score_dev", tg)) return rc;
  if (n < 0 || n > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "ww_ctc_score_dev: sequence count out of range");
  if (n == 0) return WW_OK;
  if (!d_steps || !d_score) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  WW_ON_DEVICE(ctx, dev);
  return ww_k_ctc_score(ctx, d_steps, n, T, L, tg, d_score, n, 1);
  WW_GUARD_END(ctx)
}

int ww_ctc_score_rows(const float *steps, int64_t n, int32_t T, int32_t L, const int32_t *targets, const int32_t *target_lens, int32_t K,
                      int32_t mode, float *score) {
  WW_GUARD_BEGIN
  char why[200];
  if (!ww_ctc_score_args_ok(T, L, targets, target_lens, K, mode, why, sizeof why)) return ww_fail(nullptr, WW_EINVAL, "ww_ctc_score_rows: %s", why);
  if (n < 0) return ww_fail(nullptr, WW_EINVAL, "ww_ctc_score_rows: negative sequence count");
  if (n == 0) return WW_OK;
  if (!steps || !score) return ww_fail(nullptr, WW_EINVAL, "NULL argument");
  for (int k = 0; k < K; ++k)
    for (int64_t i = 0; i < n; ++i)
      score[(size_t)k * n + i] = ww_ctc_score_row(steps + (size_t)i * T * L, T, L, L, targets + k * WW_CTC_SCORE_MAX_TARGET, target_lens[k], mode);
  return WW_OK;
  WW_GUARD_END(nullptr)
}

int ww_ctc_score(ww_ctx *ctx, const ww_model *m, const float *windows, int32_t n, const int32_t *targets, const int32_t *target_lens, int32_t K,
                 int32_t mode, float *score, int32_t max_labels, int32_t *labels, int32_t *lengths) {
  WW_GUARD_BEGIN
  ww_ctc_score_targets tg;
  if (int rc = ctc_score_check(ctx, m, targets, target_lens, K, mode, score, max_labels, labels, lengths, "ww_ctc_score", tg)) return rc;
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (n == 0) return WW_OK;
  if (!windows) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  // n stacked windows are one mel sequence of n * T rows read with hop = T
  return ctc_score_host(ctx, m, windows, (int64_t)n * m->info.window, m->info.window, n, tg, score, max_labels, labels, lengths);
  WW_GUARD_END(ctx)
}

int ww_ctc_slide_score(ww_ctx *ctx, const ww_model *m, const float *mel, int64_t rows, int32_t hop, const int32_t *targets,
                       const int32_t *target_lens, int32_t K, int32_t mode, float *score, int32_t max_labels, int32_t *labels, int32_t *lengths,
                       int64_t *n_windows) {
  WW_GUARD_BEGIN
  ww_ctc_score_targets tg;
  if (int rc = ctc_score_check(ctx, m, targets, target_lens, K, mode, score, max_labels, labels, lengths, "ww_ctc_slide_score", tg)) return rc;
  if (!n_windows) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (hop <= 0) return ww_fail(ctx, WW_EINVAL, "hop must be positive");
  if (rows < 0) return ww_fail(ctx, WW_EINVAL, "negative row count");
  const int T = m->info.window;
  const int64_t nw = rows >= T ? (rows - T) / hop + 1 : 0;
  if (nw > 0 && !mel) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  *n_windows = nw;
  if (nw == 0) return WW_OK;
  return ctc_score_host(ctx, m, mel, rows, hop, nw, tg, score, max_labels, labels, lengths);
  WW_GUARD_END(ctx)
}

int ww_ctc_score_windows_dev(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                             const int32_t *d_win_valid, int32_t n, const int32_t *targets, const int32_t *target_lens, int32_t K, int32_t mode,
                             float *d_score, int32_t max_labels, int32_t *d_labels, int32_t *d_lengths) {
  WW_GUARD_BEGIN
  ww_ctc_score_targets tg;
  if (int rc = ctc_score_check(ctx, m, targets, target_lens, K, mode, d_score, max_labels, d_labels, d_lengths, "ww_ctc_score_windows_dev", tg)) return rc;
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (n == 0) return WW_OK;
  if (!d_mel) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (!d_win_row || !d_win_valid) return ww_fail(ctx, WW_EINVAL, "window descriptors are NULL");
  WW_ON_DEVICE(ctx, dev);
  if (int rc = ww_ensure(ctx, ctx->dev, ctc_score_workspace(m, n) + 1024, false)) return rc;
  return ctc_score_chunks(ctx, m, d_mel, mel_rows, d_win_row, d_win_valid, 0, 0, n, ctx->dev.ptr, tg, d_score, max_labels, d_labels, d_lengths);
  WW_GUARD_END(ctx)
}

// ---- the Viterbi alignment (include/wwhip.h: ww_ctc_align_*; csrc/ctc_align.h): the score family's forms, one to one -------------
int ww_ctc_align_dev(ww_ctx *ctx, const float *d_steps, int64_t n, int32_t T, int32_t L, const int32_t *targets, const int32_t *target_lens,
                     int32_t K, int32_t mode, float *d_value, int8_t *d_span) {
  WW_GUARD_BEGIN
  if (!ctx) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  ww_ctc_score_targets tg;
  if (int rc = ctc_score_targets_of(ctx, T, L, targets, target_lens, K, mode, "ww_ctc_align_dev", tg)) return rc;
  if (n < 0 || n > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "ww_ctc_align_dev: sequence count out of range");
  if (!d_value || !d_span) return ww_fail(ctx, WW_EINVAL, "ww_ctc_align_dev: value / span are NULL");
  if (n == 0) return WW_OK;
  if (!d_steps) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  WW_ON_DEVICE(ctx, dev);
  return ww_k_ctc_align(ctx, d_steps, n, T, L, tg, d_value, d_span, n, 1);
  WW_GUARD_END(ctx)
}

int ww_ctc_align_rows(const float *steps, int64_t n, int32_t T, int32_t L, const int32_t *targets, const int32_t *target_lens, int32_t K,
                      int32_t mode, float *value, int8_t *span) {
  WW_GUARD_BEGIN
  char why[200];
  if (!ww_ctc_score_args_ok(T, L, targets, target_lens, K, mode, why, sizeof why)) return ww_fail(nullptr, WW_EINVAL, "ww_ctc_align_rows: %s", why);
  if (n < 0) return ww_fail(nullptr, WW_EINVAL, "ww_ctc_align_rows: negative sequence count");
  if (!value || !span) return ww_fail(nullptr, WW_EINVAL, "ww_ctc_align_rows: value / span are NULL");
  if (n == 0) return WW_OK;
  if (!steps) return ww_fail(nullptr, WW_EINVAL, "NULL argument");
  for (int k = 0; k < K; ++k)
    for (int64_t i = 0; i < n; ++i)
      ww_ctc_align_row(steps + (size_t)i * T * L, T, L, L, targets + k * WW_CTC_SCORE_MAX_TARGET, target_lens[k], mode, value + (size_t)k * n + i,
                       span + ((size_t)k * n + i) * (2 * WW_CTC_SCORE_MAX_TARGET));
  return WW_OK;
  WW_GUARD_END(nullptr)
}

int ww_ctc_align(ww_ctx *ctx, const ww_model *m, const float *windows, int32_t n, const int32_t *targets, const int32_t *target_lens, int32_t K,
                 int32_t mode, float *value, int8_t *span, int32_t max_labels, int32_t *labels, int32_t *lengths) {
  WW_GUARD_BEGIN
  ww_ctc_score_targets tg;
  if (int rc = ctc_score_check(ctx, m, targets, target_lens, K, mode, value, max_labels, labels, lengths, "ww_ctc_align", tg)) return rc;
  if (!span) return ww_fail(ctx, WW_EINVAL, "ww_ctc_align: span is NULL");
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (n == 0) return WW_OK;
  if (!windows) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  return ctc_score_host(ctx, m, windows, (int64_t)n * m->info.window, m->info.window, n, tg, nullptr, max_labels, labels, lengths, value, span);
  WW_GUARD_END(ctx)
}

int ww_ctc_slide_align(ww_ctx *ctx, const ww_model *m, const float *mel, int64_t rows, int32_t hop, const int32_t *targets,
                       const int32_t *target_lens, int32_t K, int32_t mode, float *value, int8_t *span, int32_t max_labels, int32_t *labels,
                       int32_t *lengths, int64_t *n_windows) {
  WW_GUARD_BEGIN
  ww_ctc_score_targets tg;
  if (int rc = ctc_score_check(ctx, m, targets, target_lens, K, mode, value, max_labels, labels, lengths, "ww_ctc_slide_align", tg)) return rc;
  if (!span) return ww_fail(ctx, WW_EINVAL, "ww_ctc_slide_align: span is NULL");
  if (!n_windows) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (hop <= 0) return ww_fail(ctx, WW_EINVAL, "hop must be positive");
  if (rows < 0) return ww_fail(ctx, WW_EINVAL, "negative row count");
  const int T = m->info.window;
  const int64_t nw = rows >= T ? (rows - T) / hop + 1 : 0;
  if (nw > 0 && !mel) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  *n_windows = nw;
  if (nw == 0) return WW_OK;
  return ctc_score_host(ctx, m, mel, rows, hop, nw, tg, nullptr, max_labels, labels, lengths, value, span);
  WW_GUARD_END(ctx)
}

int ww_ctc_align_windows_dev(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                             const int32_t *d_win_valid, int32_t n, const int32_t *targets, const int32_t *target_lens, int32_t K, int32_t mode,
                             float *d_value, int8_t *d_span, int32_t max_labels, int32_t *d_labels, int32_t *d_lengths) {
  WW_GUARD_BEGIN
  ww_ctc_score_targets tg;
  if (int rc = ctc_score_check(ctx, m, targets, target_lens, K, mode, d_value, max_labels, d_labels, d_lengths, "ww_ctc_align_windows_dev", tg)) return rc;
  if (!d_span) return ww_fail(ctx, WW_EINVAL, "ww_ctc_align_windows_dev: span is NULL");
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (n == 0) return WW_OK;
  if (!d_mel) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (!d_win_row || !d_win_valid) return ww_fail(ctx, WW_EINVAL, "window descriptors are NULL");
  WW_ON_DEVICE(ctx, dev);
  if (int rc = ww_ensure(ctx, ctx->dev, ctc_score_workspace(m, n) + 1024, false)) return rc;
  return ctc_score_chunks(ctx, m, d_mel, mel_rows, d_win_row, d_win_valid, 0, 0, n, ctx->dev.ptr, tg, nullptr, max_labels, d_labels, d_lengths, d_value,
                          d_span);
  WW_GUARD_END(ctx)
}

// ---- the prefix beam search (include/wwhip.h: ww_ctc_beam_*; csrc/ctc_beam.h) --------------------------------------------------------
int ww_ctc_beam_dev(ww_ctx *ctx, const float *d_steps, int64_t n, int32_t T, int32_t L, int32_t beam_width, int32_t top_paths, int32_t max_labels,
                    int32_t *d_labels, int32_t *d_lengths, float *d_prob) {
  WW_GUARD_BEGIN
  if (!ctx) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  char why[200];
  if (!ww_ctc_beam_args_ok(T, L, beam_width, top_paths, max_labels, why, sizeof why)) return ww_fail(ctx, WW_EINVAL, "ww_ctc_beam_dev: %s", why);
  if (n < 0 || n > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "ww_ctc_beam_dev: sequence count out of range");
  if (!d_labels || !d_lengths || !d_prob) return ww_fail(ctx, WW_EINVAL, "ww_ctc_beam_dev: labels / lengths / prob are NULL");
  if (n == 0) return WW_OK;
  if (!d_steps) return ww_fail(ctx, WW_EINVAL, "ww_ctc_beam_dev: steps is NULL");
  WW_ON_DEVICE(ctx, dev);
  return ww_k_ctc_beam(ctx, d_steps, n, T, L, beam_width, top_paths, max_labels, d_labels, d_lengths, d_prob);
  WW_GUARD_END(ctx)
}

int ww_ctc_beam_rows(const float *steps, int64_t n, int32_t T, int32_t L, int32_t beam_width, int32_t top_paths, int32_t max_labels,
                     int32_t *labels, int32_t *lengths, float *prob) {
  WW_GUARD_BEGIN
  char why[200];
  if (!ww_ctc_beam_args_ok(T, L, beam_width, top_paths, max_labels, why, sizeof why)) return ww_fail(nullptr, WW_EINVAL, "ww_ctc_beam_rows: %s", why);
  if (n < 0) return ww_fail(nullptr, WW_EINVAL, "ww_ctc_beam_rows: negative sequence count");
  if (!labels || !lengths || !prob) return ww_fail(nullptr, WW_EINVAL, "ww_ctc_beam_rows: labels / lengths / prob are NULL");
  if (n == 0) return WW_OK;
  if (!steps) return ww_fail(nullptr, WW_EINVAL, "ww_ctc_beam_rows: steps is NULL");
  for (int64_t i = 0; i < n; ++i)
    ww_ctc_beam_row(steps + (size_t)i * T * L, T, L, L, beam_width, top_paths, max_labels, labels + (size_t)i * top_paths * max_labels,
                    lengths + (size_t)i * top_paths, prob + (size_t)i * top_paths);
  return WW_OK;
  WW_GUARD_END(nullptr)
}

int ww_ctc_beam(ww_ctx *ctx, const ww_model *m, const float *windows, int32_t n, int32_t beam_width, int32_t top_paths, int32_t max_labels,
                int32_t *labels, int32_t *lengths, float *prob) {
  WW_GUARD_BEGIN
  if (int rc = ctc_beam_check(ctx, m, beam_width, top_paths, max_labels, labels, lengths, prob, "ww_ctc_beam")) return rc;
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (n == 0) return WW_OK;
  if (!windows) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  // n stacked windows are one mel sequence of n * T rows read with hop = T
  return ctc_beam_host(ctx, m, windows, (int64_t)n * m->info.window, m->info.window, n, beam_width, top_paths, max_labels, labels, lengths, prob);
  WW_GUARD_END(ctx)
}

int ww_ctc_slide_beam(ww_ctx *ctx, const ww_model *m, const float *mel, int64_t rows, int32_t hop, int32_t beam_width, int32_t top_paths,
                      int32_t max_labels, int32_t *labels, int32_t *lengths, float *prob, int64_t *n_windows) {
  WW_GUARD_BEGIN
  if (int rc = ctc_beam_check(ctx, m, beam_width, top_paths, max_labels, labels, lengths, prob, "ww_ctc_slide_beam")) return rc;
  if (!n_windows) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (hop <= 0) return ww_fail(ctx, WW_EINVAL, "hop must be positive");
  if (rows < 0) return ww_fail(ctx, WW_EINVAL, "negative row count");
  const int T = m->info.window;
  const int64_t nw = rows >= T ? (rows - T) / hop + 1 : 0;
  if (nw > 0 && !mel) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  *n_windows = nw;
  if (nw == 0) return WW_OK;
  return ctc_beam_host(ctx, m, mel, rows, hop, nw, beam_width, top_paths, max_labels, labels, lengths, prob);
  WW_GUARD_END(ctx)
}

int ww_ctc_beam_windows_dev(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                            const int32_t *d_win_valid, int32_t n, int32_t beam_width, int32_t top_paths, int32_t max_labels, int32_t *d_labels,
                            int32_t *d_lengths, float *d_prob) {
  WW_GUARD_BEGIN
  if (int rc = ctc_beam_check(ctx, m, beam_width, top_paths, max_labels, d_labels, d_lengths, d_prob, "ww_ctc_beam_windows_dev")) return rc;
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (n == 0) return WW_OK;
  if (!d_mel) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (!d_win_row || !d_win_valid) return ww_fail(ctx, WW_EINVAL, "window descriptors are NULL");
  WW_ON_DEVICE(ctx, dev);
  if (int rc = ww_ensure(ctx, ctx->dev, ctc_score_workspace(m, n) + 1024, false)) return rc;
  return ctc_beam_chunks(ctx, m, d_mel, mel_rows, d_win_row, d_win_valid, 0, 0, n, ctx->dev.ptr, beam_width, top_paths, max_labels, d_labels, d_lengths,
                         d_prob);
  WW_GUARD_END(ctx)
}

// ---- the forward-backward occupancy (include/wwhip.h: ww_ctc_occupancy_*; csrc/ctc_occupancy.h): the align family's forms, one to one --
int ww_ctc_occupancy_dev(ww_ctx *ctx, const float *d_steps, int64_t n, int32_t T, int32_t L, const int32_t *targets, const int32_t *target_lens,
                         int32_t K, int32_t mode, float *d_value, float *d_occ, float *d_cls) {
  WW_GUARD_BEGIN
  if (!ctx) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  char why[200];
  if (!ww_ctc_occupancy_args_ok(T, L, targets, target_lens, K, mode, d_value, d_occ, d_cls, why, sizeof why))
    return ww_fail(ctx, WW_EINVAL, "ww_ctc_occupancy_dev: %s", why);
  ww_ctc_score_targets tg;
  if (int rc = ctc_score_targets_of(ctx, T, L, targets, target_lens, K, mode, "ww_ctc_occupancy_dev", tg)) return rc;
  if (n < 0 || n > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "ww_ctc_occupancy_dev: sequence count out of range");
  if (n == 0) return WW_OK;
  if (!d_steps) return ww_fail(ctx, WW_EINVAL, "ww_ctc_occupancy_dev: steps is NULL");
  WW_ON_DEVICE(ctx, dev);
  return ww_k_ctc_occupancy(ctx, d_steps, n, T, L, tg, d_value, d_occ, d_cls, n, 1);
  WW_GUARD_END(ctx)
}

int ww_ctc_occupancy_rows(const float *steps, int64_t n, int32_t T, int32_t L, const int32_t *targets, const int32_t *target_lens, int32_t K,
                          int32_t mode, float *value, float *occ, float *cls) {
  WW_GUARD_BEGIN
  char why[200];
  if (!ww_ctc_occupancy_args_ok(T, L, targets, target_lens, K, mode, value, occ, cls, why, sizeof why))
    return ww_fail(nullptr, WW_EINVAL, "ww_ctc_occupancy_rows: %s", why);
  if (n < 0) return ww_fail(nullptr, WW_EINVAL, "ww_ctc_occupancy_rows: negative sequence count");
  if (n == 0) return WW_OK;
  if (!steps) return ww_fail(nullptr, WW_EINVAL, "ww_ctc_occupancy_rows: steps is NULL");
  for (int k = 0; k < K; ++k)
    for (int64_t i = 0; i < n; ++i) {
      const size_t o = (size_t)k * n + i;
      value[o] = ww_ctc_occupancy_row(steps + (size_t)i * T * L, T, L, L, targets + k * WW_CTC_SCORE_MAX_TARGET, target_lens[k], mode,
                                      occ + o * T * WW_CTC_SCORE_MAX_TARGET, cls ? cls + o * T * L : nullptr);
    }
  return WW_OK;
  WW_GUARD_END(nullptr)
}

int ww_ctc_occupancy(ww_ctx *ctx, const ww_model *m, const float *windows, int32_t n, const int32_t *targets, const int32_t *target_lens, int32_t K,
                     int32_t mode, float *value, float *occ, float *cls, int32_t max_labels, int32_t *labels, int32_t *lengths) {
  WW_GUARD_BEGIN
  ww_ctc_score_targets tg;
  if (int rc = ctc_occupancy_check(ctx, m, targets, target_lens, K, mode, value, occ, cls, max_labels, labels, lengths, "ww_ctc_occupancy", tg)) return rc;
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (n == 0) return WW_OK;
  if (!windows) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  // n stacked windows are one mel sequence of n * T rows read with hop = T
  return ctc_occupancy_host(ctx, m, windows, (int64_t)n * m->info.window, m->info.window, n, tg, value, occ, cls, max_labels, labels, lengths);
  WW_GUARD_END(ctx)
}

int ww_ctc_slide_occupancy(ww_ctx *ctx, const ww_model *m, const float *mel, int64_t rows, int32_t hop, const int32_t *targets,
                           const int32_t *target_lens, int32_t K, int32_t mode, float *value, float *occ, float *cls, int32_t max_labels,
                           int32_t *labels, int32_t *lengths, int64_t *n_windows) {
  WW_GUARD_BEGIN
  ww_ctc_score_targets tg;
  if (int rc = ctc_occupancy_check(ctx, m, targets, target_lens, K, mode, value, occ, cls, max_labels, labels, lengths, "ww_ctc_slide_occupancy", tg))
    return rc;
  if (!n_windows) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (hop <= 0) return ww_fail(ctx, WW_EINVAL, "hop must be positive");
  if (rows < 0) return ww_fail(ctx, WW_EINVAL, "negative row count");
  const int T = m->info.window;
  const int64_t nw = rows >= T ? (rows - T) / hop + 1 : 0;
  if (nw > 0 && !mel) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  *n_windows = nw;
  if (nw == 0) return WW_OK;
  return ctc_occupancy_host(ctx, m, mel, rows, hop, nw, tg, value, occ, cls, max_labels, labels, lengths);
  WW_GUARD_END(ctx)
}

int ww_ctc_occupancy_windows_dev(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                                 const int32_t *d_win_valid, int32_t n, const int32_t *targets, const int32_t *target_lens, int32_t K,
                                 int32_t mode, float *d_value, float *d_occ, float *d_cls, int32_t max_labels, int32_t *d_labels,
                                 int32_t *d_lengths) {
  WW_GUARD_BEGIN
  ww_ctc_score_targets tg;
  if (int rc = ctc_occupancy_check(ctx, m, targets, target_lens, K, mode, d_value, d_occ, d_cls, max_labels, d_labels, d_lengths,
                                   "ww_ctc_occupancy_windows_dev", tg))
    return rc;
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (n == 0) return WW_OK;
  if (!d_mel) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (!d_win_row || !d_win_valid) return ww_fail(ctx, WW_EINVAL, "window descriptors are NULL");
  WW_ON_DEVICE(ctx, dev);
  if (int rc = ww_ensure(ctx, ctx->dev, ctc_score_workspace(m, n) + 1024, false)) return rc;
  return ctc_occupancy_chunks(ctx, m, d_mel, mel_rows, d_win_row, d_win_valid, 0, 0, n, ctx->dev.ptr, tg, d_value, d_occ, d_cls, max_labels, d_labels,
                              d_lengths);
  WW_GUARD_END(ctx)
}

int ww_set_forward_windows_dev(ww_ctx *ctx, const ww_model_set *set, const float *d_mel, int64_t mel_rows, const int64_t *d_win_row,
                               const int32_t *d_win_valid, const int32_t *win_model, int32_t nw, float *d_out, float *d_enc) {
  WW_GUARD_BEGIN
  if (!ctx || !set) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (set->ctx != ctx) return ww_fail(ctx, WW_EINVAL, "the model set belongs to another context");
  if (nw < 0) return ww_fail(ctx, WW_EINVAL, "negative window count");
  if (nw == 0) return WW_OK;
  if (!d_mel || !d_out) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (!d_win_row || !d_win_valid || !win_model) return ww_fail(ctx, WW_EINVAL, "window descriptors are NULL");
  char why[160];
  if (int rc = ww_set_check_ids(win_model, nw, set->n, "win_model", why, sizeof why)) return ww_fail(ctx, rc, "ww_set_forward_windows_dev: %s", why);
  WW_ON_DEVICE(ctx, dev);
  const ww_model *m = &set->view;
  ww_tables tb;
  const size_t o_ids = tb.add(win_model, (size_t)nw), b_ws = model_ws(m, 1);
  if (int rc = ww_ensure(ctx, ctx->dev, tb.bytes() + b_ws + 1024, false)) return rc;
  ww_bump bump(ctx->dev.ptr, ctx->dev.cap);
  char *d_tab = bump.take<char>(tb.bytes());
  void *ws = bump.take<char>(b_ws);
  if (int rc = tb.send(ctx, d_tab)) return rc;
  ww_set_ref ref;
  ref.ids = (const int32_t *)(d_tab + o_ids);
  ref.stride = (long long)set->stride;
  return model_forward(ctx, m, d_mel, mel_rows, d_win_row, d_win_valid, 0, 0, 0, nw, ws, d_out, d_enc, &ref);
  WW_GUARD_END(ctx)
}

int ww_forward_segments_dev(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t mel_rows, const int64_t *seg_row0,
                            const int32_t *seg_nw, int32_t n_seg, int32_t hop, float *d_out) {
  WW_GUARD_BEGIN
  if (!ctx || !m || !d_mel || !d_out) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (int rc_ctc = ww_crnn_refuse_ctc(ctx, m, "ww_forward_segments_dev")) return rc_ctc;
  if (n_seg < 0) return ww_fail(ctx, WW_EINVAL, "negative sequence count");
  if (hop <= 0) return ww_fail(ctx, WW_EINVAL, "hop must be positive");
  if (n_seg == 0) return WW_OK;
  if (!seg_row0 || !seg_nw) return ww_fail(ctx, WW_EINVAL, "sequence descriptors are NULL");
  WW_ON_DEVICE(ctx, dev);
  // a bad descriptor is refused before anything is enqueued, whichever form the call takes
  const int T = m->info.window;
  int64_t nw;
  char why[WW_SEG_ERR];
  if (int rc = seg_walk(seg_row0, seg_nw, n_seg, hop, T, mel_rows, &nw, why)) return ww_fail(ctx, rc, "%s", why);
  if (ww_crnn_segments_capable(m, hop)) return ww_k_crnn_segments_forward(ctx, m, d_mel, mel_rows, seg_row0, seg_nw, n_seg, hop, d_out);
  // every other model / mode: the same windows as an explicit list through the per-window kernels
  if (nw == 0) return WW_OK;
  if (nw > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "too many windows in one call");
  std::vector<int64_t> rows;
  seg_rows(seg_row0, seg_nw, n_seg, hop, rows);
  std::vector<int32_t> valid((size_t)nw, T);
  ww_tables tb;
  const size_t o_rows = tb.add(rows), o_valid = tb.add(valid), b_ws = model_ws(m, chunk_of(nw));
  int rc = ww_ensure(ctx, ctx->dev, tb.bytes() + b_ws + 1024, false);
  if (rc) return rc;
  ww_bump bump(ctx->dev.ptr, ctx->dev.cap);
  char *d_tab = bump.take<char>(tb.bytes());
  int64_t *d_rows = (int64_t *)(d_tab + o_rows);
  int32_t *d_valid = (int32_t *)(d_tab + o_valid);
  void *ws = bump.take<char>(b_ws);
  if ((rc = tb.send(ctx, d_tab))) return rc;
  return forward_chunks(ctx, m, d_mel, mel_rows, d_rows, d_valid, 0, 0, nw, ws, d_out, nullptr, no_enc);
  WW_GUARD_END(ctx)
}

}  // extern "C"

// ---- a model set's sliding evaluation ------------------------------------------------------------------------------------------
#define WW_SET_SLOT_CHUNK 1024  // member slots per launch of the sliding form (duplicates are allowed: a call may bring any number)

// Everything ww_set_forward_segments_dev refuses, before anything is enqueued.  *W_out: windows per member, *n_slots: the call's
// member slots; WW_OK with *W_out = 0: nothing to do.
static int set_segments_check(ww_ctx *ctx, const ww_model_set *set, const void *d_mel, int64_t mel_rows, const int64_t *seg_row0,
                              const int32_t *seg_nw, int32_t n_seg, int32_t hop, const int32_t *members, int32_t n_members, const void *d_out,
                              int32_t *n_slots, int64_t *W_out) {
  *W_out = 0;
  *n_slots = 0;
  if (!ctx || !set) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (set->ctx != ctx) return ww_fail(ctx, WW_EINVAL, "the model set belongs to another context");
  if (!d_mel || !d_out) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (hop <= 0) return ww_fail(ctx, WW_EINVAL, "hop must be positive");
  if (n_seg < 0) return ww_fail(ctx, WW_EINVAL, "negative sequence count");
  if (n_members < 0) return ww_fail(ctx, WW_EINVAL, "negative member count");
  if (n_seg > 0 && (!seg_row0 || !seg_nw)) return ww_fail(ctx, WW_EINVAL, "sequence descriptors are NULL");
  int64_t W;
  char why[160];
  if (int rc = seg_walk(seg_row0, seg_nw, n_seg, hop, set->view.info.window, mel_rows, &W, why)) return ww_fail(ctx, rc, "%s", why);
  if (int rc = ww_set_check_ids(members, n_members, set->n, "members", why, sizeof why)) return ww_fail(ctx, rc, "ww_set_forward_segments_dev: %s", why);
  const int32_t slots = members ? n_members : set->n;
  if (slots == 0 || W == 0) return WW_OK;
  if (W * slots > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "too many windows in one call");
  *n_slots = slots;
  *W_out = W;
  return WW_OK;
}

// the checked call (the context's device is current)
static int set_segments_run(ww_ctx *ctx, const ww_model_set *set, const float *d_mel, int64_t mel_rows, const int64_t *seg_row0,
                            const int32_t *seg_nw, int32_t n_seg, int32_t hop, const int32_t *members, int32_t n_slots, int64_t W, float *d_out) {
  const ww_model *m = &set->view;
  const int NO = m->info.n_out, T = m->info.window;
  std::vector<int32_t> all;
  if (!members) {
    all.resize((size_t)n_slots);
    for (int k = 0; k < n_slots; ++k) all[k] = k;
    members = all.data();
  }
  if (ww_crnn_set_segments_rows_form(m, hop, W)) {
    for (int32_t k0 = 0; k0 < n_slots; k0 += WW_SET_SLOT_CHUNK) {
      const int n = n_slots - k0 < WW_SET_SLOT_CHUNK ? n_slots - k0 : WW_SET_SLOT_CHUNK;
      const ww_crnn_set_call sc = {(long long)set->stride, members + k0, n, W};
      if (int rc = ww_k_crnn_segments_forward(ctx, m, d_mel, mel_rows, seg_row0, seg_nw, n_seg, hop, d_out + (size_t)k0 * W * NO, &sc)) return rc;
    }
    return WW_OK;
  }
  // every other model / form: the same windows as an explicit list of n_slots x W descriptors naming the same rows, member-major -
  // descriptor k * W + w is window w by member members[k], and its detect row is row k * W + w of d_out
  const size_t nw = (size_t)n_slots * (size_t)W;
  std::vector<int64_t> rows;
  std::vector<int32_t> ids(nw);
  rows.reserve(nw);
  seg_rows(seg_row0, seg_nw, n_seg, hop, rows);
  rows.resize(nw);
  for (int k = 1; k < n_slots; ++k) std::copy(rows.begin(), rows.begin() + W, rows.begin() + (size_t)k * W);
  for (int k = 0; k < n_slots; ++k) std::fill(ids.begin() + (size_t)k * W, ids.begin() + (size_t)(k + 1) * W, members[k]);
  const std::vector<int32_t> valid(nw, T);
  ww_tables tb;
  const size_t o_rows = tb.add(rows), o_valid = tb.add(valid), o_ids = tb.add(ids), b_ws = model_ws(m, 1);
  if (int rc = ww_ensure(ctx, ctx->dev, tb.bytes() + b_ws + 1024, false)) return rc;
  ww_bump bump(ctx->dev.ptr, ctx->dev.cap);
  char *d_tab = bump.take<char>(tb.bytes());
  void *ws = bump.take<char>(b_ws);
  if (int rc = tb.send(ctx, d_tab)) return rc;
  ww_set_ref ref;
  ref.ids = (const int32_t *)(d_tab + o_ids);
  ref.stride = (long long)set->stride;
  const int64_t *d_rows = (const int64_t *)(d_tab + o_rows);
  const int32_t *d_valid = (const int32_t *)(d_tab + o_valid);
  return model_forward(ctx, m, d_mel, mel_rows, d_rows, d_valid, 0, 0, 0, (int)nw, ws, d_out, nullptr, &ref);
}

extern "C" {

int ww_set_forward_segments_dev(ww_ctx *ctx, const ww_model_set *set, const float *d_mel, int64_t mel_rows, const int64_t *seg_row0,
                                const int32_t *seg_nw, int32_t n_seg, int32_t hop, const int32_t *members, int32_t n_members, float *d_out) {
  WW_GUARD_BEGIN
  int32_t n_slots;
  int64_t W;
  if (int rc = set_segments_check(ctx, set, d_mel, mel_rows, seg_row0, seg_nw, n_seg, hop, members, n_members, d_out, &n_slots, &W)) return rc;
  if (W == 0) return WW_OK;
  WW_ON_DEVICE(ctx, dev);
  return set_segments_run(ctx, set, d_mel, mel_rows, seg_row0, seg_nw, n_seg, hop, members, n_slots, W, d_out);
  WW_GUARD_END(ctx)
}

int ww_set_slide_forward(ww_ctx *ctx, const ww_model_set *set, const float *mel, int64_t rows, int32_t hop, const int32_t *members,
                         int32_t n_members, float *out, int64_t *n_windows) {
  WW_GUARD_BEGIN
  if (!ctx || !set || !n_windows) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (hop <= 0) return ww_fail(ctx, WW_EINVAL, "hop must be positive");
  if (rows < 0) return ww_fail(ctx, WW_EINVAL, "negative row count");
  const int T = set->view.info.window, F = set->view.info.n_mel, NO = set->view.info.n_out;
  const int64_t nw = rows >= T ? (rows - T) / hop + 1 : 0;
  if (nw > 0x7fffffff) return ww_fail(ctx, WW_EINVAL, "too many windows in one call");
  *n_windows = nw;
  if (nw > 0 && (!mel || !out)) return ww_fail(ctx, WW_EINVAL, "NULL buffer");
  const int64_t row0 = 0;
  const int32_t seg_nw = (int32_t)nw;
  int32_t n_slots;
  int64_t W;
  // (the same checks on the caller's own pointers: what is refused is refused before a byte moves; without a window there is no buffer
  // to name)
  if (int rc = set_segments_check(ctx, set, nw ? (const void *)mel : (const void *)&row0, rows, &row0, &seg_nw, 1, hop, members, n_members,
                                  nw ? (const void *)out : (const void *)&row0, &n_slots, &W))
    return rc;
  if (W == 0) return WW_OK;
  WW_ON_DEVICE(ctx, dev);
  // the sequence and the detect rows in one allocation of the call's own (the launchers carve the context's arena from its start)
  const size_t b_mel = ww_bump::need((size_t)rows * F, 4), b_out = ww_bump::need((size_t)n_slots * W * NO, 4);
  struct dev_block {
    void *p = nullptr;
    ~dev_block() {
      if (p) (void)hipFree(p);
    }
  } blk;
  if (hipMalloc(&blk.p, b_mel + b_out) != hipSuccess) {
    blk.p = nullptr;
    return ww_fail(ctx, WW_ENOMEM, "ww_set_slide_forward: cannot allocate %zu bytes of device memory", b_mel + b_out);
  }
  float *d_mel = (float *)blk.p, *d_out = (float *)((char *)blk.p + b_mel);
  int rc = WW_OK;
  hipError_t e = hipMemcpyAsync(d_mel, mel, (size_t)rows * F * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    rc = set_segments_run(ctx, set, d_mel, rows, &row0, &seg_nw, 1, hop, members, n_slots, W, d_out);
    if (rc == WW_OK) e = hipMemcpyAsync(out, d_out, (size_t)n_slots * W * NO * 4, hipMemcpyDeviceToHost, ctx->stream);
  }
  // the block is freed behind this wait, whatever the status
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (rc == WW_OK && (e != hipSuccess || es != hipSuccess))
    rc = ww_fail(ctx, WW_EHIP, "ww_set_slide_forward: %s", hipGetErrorString(e != hipSuccess ? e : es));
  return rc;
  WW_GUARD_END(ctx)
}

}  // extern "C"

// ---- the Wavenet's sequence form (wavenet.hip: wavenet_seq_kernel), for a model and for a model set --------------------------------
// One shape for the six entry points.  set == NULL: a single model - one plane, no ids.  Otherwise m is the set's view and, by_seq:
// ONE plane, sequence s by member ids[s] (n_ids = n_seq; ids == NULL: member 0); else plane k by member ids[k] (ids == NULL: every
// member in order, n_ids only checked for its sign).
struct wave_seq_request {
  const ww_model *m;
  const ww_model_set *set;
  const float *mel;  // host or device, as the entry point's outputs
  int64_t total_rows;
  const int64_t *row_offs;
  int32_t n_seq, pool_rows;
  const int32_t *ids;
  int32_t n_ids;
  bool by_seq;
  float *enc, *logits, *pf, *post;
};

static int wave_seq_validate(ww_ctx *ctx, int64_t total_rows, const int64_t *row_offs, int32_t n_seq, int32_t pool_rows) {
  if (n_seq < 0) return ww_fail(ctx, WW_EINVAL, "negative sequence count");
  if (pool_rows < 0) return ww_fail(ctx, WW_EINVAL, "negative pool length");
  if (total_rows < 0) return ww_fail(ctx, WW_EINVAL, "negative row count");
  if (n_seq == 0) return WW_OK;
  if (!row_offs) return ww_fail(ctx, WW_EINVAL, "row_offs is NULL");
  if (row_offs[0] < 0 || row_offs[n_seq] > total_rows) return ww_fail(ctx, WW_EINVAL, "row_offs leave the mel buffer");
  for (int s = 0; s < n_seq; ++s)
    if (row_offs[s + 1] < row_offs[s]) return ww_fail(ctx, WW_EINVAL, "row_offs descend at sequence %d", s);
  return WW_OK;
}

// Everything the six refuse, before anything is enqueued or written.  *slots: the call's planes (no set, by_seq: 1); 0 with WW_OK: a no-op
static int wave_seq_check(ww_ctx *ctx, const wave_seq_request &c, const char *what, int32_t *slots) {
  *slots = 0;
  if (!ctx || !c.m) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (c.set && c.set->ctx != ctx) return ww_fail(ctx, WW_EINVAL, "the model set belongs to another context");
  if (int rc = ww_crnn_refuse_ctc(ctx, c.m, what)) return rc;
  if (int rc = ww_wave_seq_check(ctx, c.m, what)) return rc;
  if (int rc = wave_seq_validate(ctx, c.total_rows, c.row_offs, c.n_seq, c.pool_rows)) return rc;
  if (c.set) {
    if (c.n_ids < 0) return ww_fail(ctx, WW_EINVAL, "negative member count");
    char why[160];
    if (int rc = ww_set_check_ids(c.ids, c.n_ids, c.set->n, c.by_seq ? "seq_model" : "members", why, sizeof why)) return ww_fail(ctx, rc, "%s: %s", what, why);
  }
  const int32_t n = !c.set || c.by_seq ? 1 : c.ids ? c.n_ids : c.set->n;
  if (c.n_seq == 0 || c.row_offs[c.n_seq] == c.row_offs[0] || n == 0) return WW_OK;
  if (!c.mel) return ww_fail(ctx, WW_EINVAL, "NULL mel buffer");
  if (!c.enc && !c.logits && !c.pf && !c.post) return WW_OK;
  *slots = n;
  return WW_OK;
}

// The plan of a launch of `planes` planes: the model gives the receptive field, the width of a logit row and the segment option
// (which outputs exist decides the plan's scratch, not where they are)
static void wave_seq_plan_of(const wave_seq_request &c, int planes, wave_seq_plan &pl) {
  wave_seq_make_plan(ww_wave_receptive_field(c.m), c.m->info.n_out, c.m->opt_wave_seq_segment, c.total_rows, c.row_offs, c.n_seq, planes,
                     !c.set ? WAVE_SEQ_IDS_NONE : c.by_seq ? WAVE_SEQ_IDS_BY_SEQ : WAVE_SEQ_IDS_BY_PLANE, !c.logits && (c.pf || c.post),
                     c.pf != nullptr, pl);
}
static int wave_seq_planes(int32_t slots) { return slots < WW_SET_SLOT_CHUNK ? slots : WW_SET_SLOT_CHUNK; }

// The checked call on DEVICE buffers (the context's device is current): one launch of the model kernel per WW_SET_SLOT_CHUNK slots
// - the plane is a 16-bit grid dimension, and the scratch of a call with many duplicates stays bounded.  `bump`: the arena behind
// what the caller took from it; the caller has reserved the first launch's plan there (the largest).  Each launch's tables are ONE
// block: segments, row_offs and, of a set, the launch's ids and (by_seq) the sequence of each segment.
static int wave_seq_run(ww_ctx *ctx, const wave_seq_request &c, int32_t slots, const wave_seq_plan &first, ww_bump bump) {
  const int NO = c.m->info.n_out, S = c.m->info.enc_width;
  const size_t rows = (size_t)c.total_rows;
  std::vector<int32_t> own;
  const int32_t *ids = c.ids;
  if (c.set && !ids) {
    own.assign(c.by_seq ? (size_t)c.n_seq : (size_t)slots, 0);  // (every sequence by member 0)
    if (!c.by_seq)
      for (int32_t k = 0; k < slots; ++k) own[k] = k;
    ids = own.data();
  }
  for (int32_t k0 = 0; k0 < slots; k0 += WW_SET_SLOT_CHUNK) {
    const int planes = wave_seq_planes(slots - k0);
    wave_seq_plan later;
    if (k0) wave_seq_plan_of(c, planes, later);
    const wave_seq_plan &pl = k0 ? later : first;
    if (pl.segs.empty()) return WW_OK;
    if (pl.segs.size() > 0x7fffffffu) return ww_fail(ctx, WW_EINVAL, "too many segments in one call");
    ww_tables tb;
    const size_t o_segs = tb.add(pl.segs), o_offs = tb.add(c.row_offs, (size_t)c.n_seq + 1);
    const size_t o_ids = c.set ? tb.add(c.by_seq ? ids : ids + k0, c.by_seq ? (size_t)c.n_seq : (size_t)planes) : 0;
    const size_t o_aux = c.set && c.by_seq ? tb.add(pl.seg_seq) : 0;
    if (tb.bytes() != pl.b_segs + pl.b_offs + pl.b_ids + pl.b_aux) return ww_fail(ctx, WW_EINTERNAL, "wave_seq_run: the tables are not the size the plan reserved");
    ww_bump scratch = bump;  // (the launches of a call follow each other on one stream: they share the scratch)
    char *d_tab = scratch.take<char>(tb.bytes());
    const size_t at = (size_t)k0 * rows;  // the launch's first plane, in rows
    float *d_pf = c.pf ? c.pf + at * NO : nullptr, *d_post = c.post ? c.post + (size_t)k0 * c.n_seq * NO : nullptr;
    float *d_z = c.logits ? c.logits + at * NO : nullptr;
    if (!d_z && (d_pf || d_post)) d_z = scratch.take<float>(planes * rows * NO);
    float *d_a = d_pf ? scratch.take<float>(planes * rows * NO) : nullptr, *d_b = d_pf ? scratch.take<float>(planes * rows * NO) : nullptr;
    if (int rc = tb.send(ctx, d_tab)) return rc;
    ww_set_ref ref;
    if (c.set) ref = {(const int32_t *)(d_tab + o_ids), c.by_seq ? (const int32_t *)(d_tab + o_aux) : nullptr, (long long)c.set->stride};
    if (int rc = ww_k_wave_sequence(ctx, c.m, c.mel, (const wv_seg *)(d_tab + o_segs), (int)pl.segs.size(), c.enc ? c.enc + at * S : nullptr, d_z,
                                    c.set ? &ref : nullptr, planes, c.total_rows))
      return rc;
    if (d_pf || d_post)
      if (int rc = ww_k_wave_pool(ctx, d_z, c.row_offs[c.n_seq] - c.row_offs[0], c.row_offs[c.n_seq], NO, (const int64_t *)(d_tab + o_offs), c.n_seq,
                                  c.pool_rows, pl.max_len, d_a, d_b, d_pf, d_post, planes, c.total_rows))
        return rc;
  }
  return WW_OK;
}

static int wave_seq_dev(ww_ctx *ctx, const wave_seq_request &c, const char *what) {
  int32_t slots;
  if (int rc = wave_seq_check(ctx, c, what, &slots)) return rc;
  if (slots == 0) return WW_OK;
  WW_ON_DEVICE(ctx, dev);
  wave_seq_plan pl;
  wave_seq_plan_of(c, wave_seq_planes(slots), pl);
  if (int rc = ww_ensure(ctx, ctx->dev, pl.bytes() + 1024, false)) return rc;
  return wave_seq_run(ctx, c, slots, pl, ww_bump(ctx->dev.ptr, ctx->dev.cap));
}

// HOST buffers: one upload of the mel, the outputs' planes on the device, every plane's sequence rows back.  Synchronous.
static int wave_seq_host(ww_ctx *ctx, const wave_seq_request &c, const char *what) {
  int32_t slots;
  if (int rc = wave_seq_check(ctx, c, what, &slots)) return rc;
  if (slots == 0) return WW_OK;
  WW_ON_DEVICE(ctx, dev);
  const int F = c.m->info.n_mel, NO = c.m->info.n_out, S = c.m->info.enc_width;
  const size_t rows = (size_t)c.total_rows, K = (size_t)slots;
  wave_seq_plan pl;
  wave_seq_plan_of(c, wave_seq_planes(slots), pl);
  wave_seq_request d = c;
  const size_t b_mel = ww_bump::need(rows * F, 4), b_enc = c.enc ? ww_bump::need(K * rows * S, 4) : 0, b_rows = ww_bump::need(K * rows * NO, 4);
  const size_t b_post = ww_bump::need(K * c.n_seq * NO, 4);
  if (int rc = ww_ensure(ctx, ctx->dev, b_mel + b_enc + 2 * b_rows + b_post + pl.bytes() + 1024, false)) return rc;
  ww_bump bump(ctx->dev.ptr, ctx->dev.cap);
  float *d_mel = bump.take<float>(rows * F);
  d.mel = d_mel;
  d.enc = c.enc ? bump.take<float>(K * rows * S) : nullptr;
  d.logits = c.logits ? bump.take<float>(K * rows * NO) : nullptr;
  d.pf = c.pf ? bump.take<float>(K * rows * NO) : nullptr;
  d.post = c.post ? bump.take<float>(K * c.n_seq * NO) : nullptr;
  // rows of the mel buffer outside every sequence are never read, rows of the outputs outside every sequence never written, in any
  // plane: only [r0, r1) travels, each way, and the caller's bytes elsewhere stay as they are
  const int64_t r0 = c.row_offs[0], r1 = c.row_offs[c.n_seq];
  WW_HIP(ctx, hipMemcpyAsync(d_mel + r0 * F, c.mel + r0 * F, (size_t)(r1 - r0) * F * 4, hipMemcpyHostToDevice, ctx->stream));
  if (d.post) WW_HIP(ctx, hipMemcpyAsync(d.post, c.post, K * c.n_seq * NO * 4, hipMemcpyHostToDevice, ctx->stream));  // (empty sequences keep theirs)
  if (int rc = wave_seq_run(ctx, d, slots, pl, bump)) return rc;
  for (size_t k = 0; k < K; ++k) {
    const size_t p = k * rows;
    if (c.enc) WW_HIP(ctx, hipMemcpyAsync(c.enc + (p + r0) * S, d.enc + (p + r0) * S, (size_t)(r1 - r0) * S * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (c.logits) WW_HIP(ctx, hipMemcpyAsync(c.logits + (p + r0) * NO, d.logits + (p + r0) * NO, (size_t)(r1 - r0) * NO * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (c.pf) WW_HIP(ctx, hipMemcpyAsync(c.pf + (p + r0) * NO, d.pf + (p + r0) * NO, (size_t)(r1 - r0) * NO * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (c.post) WW_HIP(ctx, hipMemcpyAsync(c.post, d.post, K * c.n_seq * NO * 4, hipMemcpyDeviceToHost, ctx->stream));
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return WW_OK;
}

extern "C" {

int ww_wave_sequence_dev(ww_ctx *ctx, const ww_model *m, const float *d_mel, int64_t total_rows, const int64_t *row_offs, int32_t n_seq,
                         int32_t pool_rows, float *d_enc, float *d_logits, float *d_post_frames, float *d_post) {
  WW_GUARD_BEGIN
  const wave_seq_request c = {m, nullptr, d_mel, total_rows, row_offs, n_seq, pool_rows, nullptr, 0, false, d_enc, d_logits, d_post_frames, d_post};
  return wave_seq_dev(ctx, c, "ww_wave_sequence_dev");
  WW_GUARD_END(ctx)
}

int ww_wave_sequence(ww_ctx *ctx, const ww_model *m, const float *mel, int64_t total_rows, const int64_t *row_offs, int32_t n_seq,
                     int32_t pool_rows, float *enc, float *logits, float *post_frames, float *post) {
  WW_GUARD_BEGIN
  const wave_seq_request c = {m, nullptr, mel, total_rows, row_offs, n_seq, pool_rows, nullptr, 0, false, enc, logits, post_frames, post};
  return wave_seq_host(ctx, c, "ww_wave_sequence");
  WW_GUARD_END(ctx)
}

int ww_set_wave_sequence_dev(ww_ctx *ctx, const ww_model_set *set, const float *d_mel, int64_t total_rows, const int64_t *row_offs, int32_t n_seq,
                             const int32_t *seq_model, int32_t pool_rows, float *d_enc, float *d_logits, float *d_post_frames, float *d_post) {
  WW_GUARD_BEGIN
  const wave_seq_request c = {set ? &set->view : nullptr, set, d_mel, total_rows, row_offs, n_seq, pool_rows, seq_model, n_seq < 0 ? 0 : n_seq, true, d_enc, d_logits, d_post_frames, d_post};
  return wave_seq_dev(ctx, c, "ww_set_wave_sequence_dev");
  WW_GUARD_END(ctx)
}

int ww_set_wave_sequence(ww_ctx *ctx, const ww_model_set *set, const float *mel, int64_t total_rows, const int64_t *row_offs, int32_t n_seq,
                         const int32_t *seq_model, int32_t pool_rows, float *enc, float *logits, float *post_frames, float *post) {
  WW_GUARD_BEGIN
  const wave_seq_request c = {set ? &set->view : nullptr, set, mel, total_rows, row_offs, n_seq, pool_rows, seq_model, n_seq < 0 ? 0 : n_seq, true, enc, logits, post_frames, post};
  return wave_seq_host(ctx, c, "ww_set_wave_sequence");
  WW_GUARD_END(ctx)
}

int ww_set_wave_sequence_all_dev(ww_ctx *ctx, const ww_model_set *set, const float *d_mel, int64_t total_rows, const int64_t *row_offs, int32_t n_seq,
                                 int32_t pool_rows, const int32_t *members, int32_t n_members, float *d_enc, float *d_logits, float *d_post_frames,
                                 float *d_post) {
  WW_GUARD_BEGIN
  const wave_seq_request c = {set ? &set->view : nullptr, set, d_mel, total_rows, row_offs, n_seq, pool_rows, members, n_members, false, d_enc, d_logits, d_post_frames, d_post};
  return wave_seq_dev(ctx, c, "ww_set_wave_sequence_all_dev");
  WW_GUARD_END(ctx)
}

int ww_set_wave_sequence_all(ww_ctx *ctx, const ww_model_set *set, const float *mel, int64_t total_rows, const int64_t *row_offs, int32_t n_seq,
                             int32_t pool_rows, const int32_t *members, int32_t n_members, float *enc, float *logits, float *post_frames, float *post) {
  WW_GUARD_BEGIN
  const wave_seq_request c = {set ? &set->view : nullptr, set, mel, total_rows, row_offs, n_seq, pool_rows, members, n_members, false, enc, logits, post_frames, post};
  return wave_seq_host(ctx, c, "ww_set_wave_sequence_all");
  WW_GUARD_END(ctx)
}

int ww_clips_forward_dev(ww_ctx *ctx, const ww_model *m, const int16_t *d_pcm, int32_t n_clips, int32_t samples,
                         const ww_frontend_params *fp, float *d_out) {
  WW_GUARD_BEGIN
  if (!ctx || !m || !d_pcm || !d_out) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (int rc_ctc = ww_crnn_refuse_ctc(ctx, m, "ww_clips_forward_dev")) return rc_ctc;
  if (n_clips < 0 || samples < 0) return ww_fail(ctx, WW_EINVAL, "negative size");
  if (n_clips == 0) return WW_OK;
  if (n_clips > 65535) return ww_fail(ctx, WW_EINVAL, "at most 65535 clips per call");
  if (((uintptr_t)d_pcm & 15) != 0) return ww_fail(ctx, WW_EINVAL, "d_pcm must be 16-byte aligned");
  int rc = check_fp(ctx, fp, true);
  if (rc) return rc;
  WW_ON_DEVICE(ctx, dev);
  const int64_t nf = ww_num_frames(samples, fp->hop);
  const int F = m->info.n_mel, T = m->info.window;
  // offset tables for this batch geometry: built once, outside any capture
  int64_t *d_so = nullptr, *d_fo = nullptr;
  for (auto &co : ctx->clip_offs)
    if (co.n_clips == n_clips && co.samples == samples && co.hop == fp->hop) {
      d_so = co.d_so;
      d_fo = co.d_fo;
    }
  if (!d_so) {
    // at most eight geometries stay cached (two small tables each); the oldest goes once nothing enqueued can still read it
    if (ctx->clip_offs.size() >= 8) {
      WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
      hipFree(ctx->clip_offs.front().d_so);
      hipFree(ctx->clip_offs.front().d_fo);
      ctx->clip_offs.erase(ctx->clip_offs.begin());
    }
    ww_ctx::clip_offs_t co;
    co.n_clips = n_clips; co.samples = samples; co.hop = fp->hop;
    WW_HIP(ctx, hipMalloc((void **)&co.d_so, sizeof(int64_t) * (n_clips + 1)));
    WW_HIP(ctx, hipMalloc((void **)&co.d_fo, sizeof(int64_t) * (n_clips + 1)));
    hipLaunchKernelGGL(iota_offs_kernel, dim3((n_clips + 256) / 256), dim3(256), 0, ctx->stream, co.d_so, co.d_fo, n_clips,
                       (int64_t)samples, nf);
    WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->clip_offs.push_back(co);
    d_so = co.d_so;
    d_fo = co.d_fo;
  }
  // workspace: mel | model scratch
  const size_t b_mel = ww_bump::need((size_t)n_clips * (nf > 0 ? nf : 1) * F, 4);
  const size_t b_ws = model_ws(m, n_clips);
  if ((rc = ww_ensure(ctx, ctx->dev, b_mel + b_ws + 1024, false))) return rc;
  ww_bump bump(ctx->dev.ptr, ctx->dev.cap);
  float *d_mel = bump.take<float>((size_t)n_clips * (nf > 0 ? nf : 1) * F);
  void *ws = bump.take<char>(b_ws);
  // Plain stream launches: measured on MI355X (round 1) the chain replays slower as a hipGraph (93 vs 88 us: the queue stays
  // full, so launch latency is hidden, while a graph replay has a 10-16 us floor).
  if ((rc = ww_k_logmel(ctx, m, d_pcm, nullptr, d_so, d_fo, n_clips, (int64_t)n_clips * nf, nf, fp, d_mel, samples, (int64_t)n_clips * samples)))
    return rc;
  // one window per clip: rows [c*nf, c*nf + min(nf, T)), zero padded to T
  return model_forward(ctx, m, d_mel, (int64_t)n_clips * nf, nullptr, nullptr, 0, (int)nf, (int)(nf < T ? nf : T), n_clips, ws, d_out,
                       nullptr);
  WW_GUARD_END(ctx)
}

// ------------------------------------------------------------------------------------------
// posterior smoothing + sweep
// ------------------------------------------------------------------------------------------
// pos / neg: host pointers (uploaded here) or, with on_device, device pointers the kernels read where they are
static int far_frr_impl(ww_ctx *ctx, bool on_device, const float *pos, int64_t n_pos, const float *neg, int64_t n_neg, int32_t win,
                        const double *thr, int32_t n_thr, double num_wakewords, double hours, double *frr, double *fa_per_h,
                        int64_t *fa_count, double *smoothed_host, double *smoothed_dev) {
  if (!ctx || !thr || !frr || !fa_per_h) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (n_pos < 0 || n_neg < 0 || n_thr <= 0) return ww_fail(ctx, WW_EINVAL, "bad sizes");
  if ((n_pos && !pos) || (n_neg && !neg)) return ww_fail(ctx, WW_EINVAL, "NULL posterior buffer");
  if (win > 0 && n_neg > 0 && n_neg < win)
    return ww_fail(ctx, WW_EINVAL, "negative stream shorter than the smoothing window (np.convolve 'same' would change its length)");
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  const size_t b_p = on_device ? 0 : ww_bump::need((size_t)n_pos + 1, 4), b_n = on_device ? 0 : ww_bump::need((size_t)n_neg + 1, 4);
  const size_t b_s = smoothed_dev ? 0 : ww_bump::need((size_t)n_neg + 1, 8), b_t = ww_bump::need((size_t)n_thr, 8);
  int rc = ww_ensure(ctx, ctx->dev, b_p + b_n + b_s + 3 * b_t + 1024, false);
  if (rc) return rc;
  ww_bump bump(ctx->dev.ptr, ctx->dev.cap);
  const float *d_pos = pos, *d_neg = neg;
  if (!on_device) {
    float *up = bump.take<float>(n_pos + 1), *un = bump.take<float>(n_neg + 1);
    if (n_pos) WW_HIP(ctx, hipMemcpyAsync(up, pos, (size_t)n_pos * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n_neg) WW_HIP(ctx, hipMemcpyAsync(un, neg, (size_t)n_neg * 4, hipMemcpyHostToDevice, ctx->stream));
    d_pos = up;
    d_neg = un;
  }
  double *d_sm = smoothed_dev ? smoothed_dev : bump.take<double>(n_neg + 1), *d_thr = bump.take<double>(n_thr);
  unsigned long long *d_pc = bump.take<unsigned long long>(n_thr), *d_fc = bump.take<unsigned long long>(n_thr);
  WW_HIP(ctx, hipMemcpyAsync(d_thr, thr, (size_t)n_thr * 8, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = ww_k_far_frr(ctx, d_pos, n_pos, d_neg, n_neg, win, d_thr, n_thr, d_sm, d_pc, d_fc))) return rc;
  std::vector<unsigned long long> pc(n_thr), fc(n_thr);
  WW_HIP(ctx, hipMemcpyAsync(pc.data(), d_pc, (size_t)n_thr * 8, hipMemcpyDeviceToHost, ctx->stream));
  WW_HIP(ctx, hipMemcpyAsync(fc.data(), d_fc, (size_t)n_thr * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (smoothed_host && n_neg) WW_HIP(ctx, hipMemcpyAsync(smoothed_host, d_sm, (size_t)n_neg * 8, hipMemcpyDeviceToHost, ctx->stream));
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < n_thr; ++k) {
    frr[k] = (num_wakewords - (double)pc[k]) / num_wakewords;
    fa_per_h[k] = (double)fc[k] / hours;
    if (fa_count) fa_count[k] = (int64_t)fc[k];
  }
  return WW_OK;
}

int ww_far_frr(ww_ctx *ctx, const float *pos, int64_t n_pos, const float *neg, int64_t n_neg, int32_t win,
               const double *thr, int32_t n_thr, double num_wakewords, double hours, double *frr, double *fa_per_h,
               int64_t *fa_count, double *smoothed) {
  WW_GUARD_BEGIN
  return far_frr_impl(ctx, false, pos, n_pos, neg, n_neg, win, thr, n_thr, num_wakewords, hours, frr, fa_per_h, fa_count, smoothed, nullptr);
  WW_GUARD_END(ctx)
}

int ww_far_frr_dev(ww_ctx *ctx, const float *d_pos, int64_t n_pos, const float *d_neg, int64_t n_neg, int32_t win,
                   const double *thr, int32_t n_thr, double num_wakewords, double hours, double *frr, double *fa_per_h,
                   int64_t *fa_count, double *d_smoothed) {
  WW_GUARD_BEGIN
  return far_frr_impl(ctx, true, d_pos, n_pos, d_neg, n_neg, win, thr, n_thr, num_wakewords, hours, frr, fa_per_h, fa_count, nullptr, d_smoothed);
  WW_GUARD_END(ctx)
}

int ww_posterior_pick_dev(ww_ctx *ctx, const float *d_rows, int64_t n, int32_t n_out, int32_t pidx, const int64_t *d_seg_offs,
                          int64_t n_seg, float *d_out) {
  WW_GUARD_BEGIN
  if (!ctx) return WW_EINVAL;
  if (n < 0 || n_seg < 0 || n_out <= 0 || pidx < 0 || pidx >= n_out) return ww_fail(ctx, WW_EINVAL, "posterior pick: bad sizes");
  if ((n > 0 && !d_rows) || ((d_seg_offs ? n_seg : n) > 0 && !d_out)) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  return ww_k_posterior_pick(ctx, d_rows, n, n_out, pidx, d_seg_offs, n_seg, d_out);
  WW_GUARD_END(ctx)
}

// ------------------------------------------------------------------------------------------
// detection events (events_plan.h: checks, geometry, scratch; posterior.hip: the five passes)
// ------------------------------------------------------------------------------------------
// post: a host pointer (uploaded here) or, with on_device, a device pointer the kernels read where it is
static int posterior_events_impl(ww_ctx *ctx, bool on_device, const float *post, int64_t n, int32_t planes, const int64_t *seg_offs,
                                 int64_t n_seg, int32_t win, const double *thr, ww_event *events, int64_t cap, int64_t *n_events,
                                 int64_t *plane_counts) {
  if (!ctx) return ww_fail(ctx, WW_EINVAL, "posterior events: NULL context");
  char why[256] = {0};
  if (ev_check(post, n, planes, seg_offs, n_seg, thr, events, cap, n_events, why, sizeof why)) return ww_fail(ctx, WW_EINVAL, "posterior events: %s", why);
  ev_plan p;
  if (ev_make_plan(n, planes, seg_offs != nullptr, n_seg, cap, p, why, sizeof why)) return ww_fail(ctx, WW_EINVAL, "posterior events: %s", why);
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  const size_t rows = (size_t)planes * (size_t)n;
  const size_t b_up = on_device ? 0 : ww_bump::need(rows + 1, 4);
  int rc = ww_ensure(ctx, ctx->dev, b_up + p.bytes + 1024, false);
  if (rc) return rc;
  ww_bump bump(ctx->dev.ptr, ctx->dev.cap);
  const float *d_post = post;
  if (!on_device) {
    float *up = bump.take<float>(rows + 1);
    if (rows) WW_HIP(ctx, hipMemcpyAsync(up, post, rows * 4, hipMemcpyHostToDevice, ctx->stream));
    d_post = up;
  }
  char *ws = bump.take<char>(p.bytes);
  const int64_t whole[2] = {0, n};  // (read by the copy below; the call ends in a synchronise)
  WW_HIP(ctx, hipMemcpyAsync(ws + p.o_offs, seg_offs ? seg_offs : whole, (size_t)p.n_offs * 8, hipMemcpyHostToDevice, ctx->stream));
  WW_HIP(ctx, hipMemcpyAsync(ws + p.o_thr, thr, (size_t)planes * 8, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = ww_k_posterior_events(ctx, d_post, p, win, ws))) return rc;
  int64_t totals[WW_EVENTS_MAX_PLANES];
  WW_HIP(ctx, hipMemcpyAsync(totals, ws + p.o_totals, (size_t)planes * 8, hipMemcpyDeviceToHost, ctx->stream));
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int64_t total = 0;
  for (int k = 0; k < planes; ++k) total += totals[k];
  const int64_t written = ev_written(total, cap);
  if (total < 0 || written > p.dev_cap) return ww_fail(ctx, WW_EINTERNAL, "posterior events: %lld events do not fit the plan's %lld", (long long)written, (long long)p.dev_cap);
  if (written > 0) {  // only the events themselves cross the bus
    WW_HIP(ctx, hipMemcpyAsync(events, ws + p.o_events, (size_t)written * sizeof(ww_event), hipMemcpyDeviceToHost, ctx->stream));
    WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  *n_events = total;
  if (plane_counts)
    for (int k = 0; k < planes; ++k) plane_counts[k] = totals[k];
  return WW_OK;
}

int ww_posterior_events_dev(ww_ctx *ctx, const float *d_post, int64_t n, int32_t planes, const int64_t *seg_offs, int64_t n_seg,
                            int32_t win, const double *thr, ww_event *events, int64_t cap, int64_t *n_events, int64_t *plane_counts) {
  WW_GUARD_BEGIN
  return posterior_events_impl(ctx, true, d_post, n, planes, seg_offs, n_seg, win, thr, events, cap, n_events, plane_counts);
  WW_GUARD_END(ctx)
}

int ww_posterior_events(ww_ctx *ctx, const float *post, int64_t n, int32_t planes, const int64_t *seg_offs, int64_t n_seg, int32_t win,
                        const double *thr, ww_event *events, int64_t cap, int64_t *n_events, int64_t *plane_counts) {
  WW_GUARD_BEGIN
  return posterior_events_impl(ctx, false, post, n, planes, seg_offs, n_seg, win, thr, events, cap, n_events, plane_counts);
  WW_GUARD_END(ctx)
}

int ww_superframe_smooth(ww_ctx *ctx, const float *in, int64_t n, int32_t T, float stay_bonus, int32_t in_is_cost,
                         uint8_t *path, uint8_t *wake) {
  WW_GUARD_BEGIN
  if (!ctx || (n > 0 && (!in || !wake))) return ww_fail(ctx, WW_EINVAL, "NULL argument");
  if (n < 0) return ww_fail(ctx, WW_EINVAL, "bad sizes");
  if (n == 0) return WW_OK;
  WW_ON_DEVICE(ctx, dev_scope);  // the caller's current device is left as it was
  const size_t b_in = ww_bump::need((size_t)n * T * 2, 4), b_p = ww_bump::need((size_t)n * T, 1), b_w = ww_bump::need((size_t)n, 1);
  int rc = ww_ensure(ctx, ctx->dev, b_in + b_p + b_w + 1024, false);
  if (rc) return rc;
  ww_bump bump(ctx->dev.ptr, ctx->dev.cap);
  float *d_in = bump.take<float>((size_t)n * T * 2);
  unsigned char *d_p = bump.take<unsigned char>((size_t)n * T), *d_w = bump.take<unsigned char>((size_t)n);
  WW_HIP(ctx, hipMemcpyAsync(d_in, in, (size_t)n * T * 2 * 4, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = ww_k_viterbi2(ctx, d_in, n, T, stay_bonus, in_is_cost, d_p, d_w))) return rc;
  if (path) WW_HIP(ctx, hipMemcpyAsync(path, d_p, (size_t)n * T, hipMemcpyDeviceToHost, ctx->stream));
  WW_HIP(ctx, hipMemcpyAsync(wake, d_w, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  WW_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return WW_OK;
  WW_GUARD_END(ctx)
}

}  // extern "C"
