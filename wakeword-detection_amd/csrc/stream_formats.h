// stream_formats.h - the host-only bookkeeping of a stream bank whose rate classes read their frames and packets in a sample format of
// their own: int16, or G.711 mu-law / A-law at one byte per sample (include/wwhip.h: ww_stream_attach_rates_fmt,
// ww_stream_attach_resampler_fmt).  Plain C++ on top of stream_rates.h (no HIP header, no HIP call): common.h includes
// it for the .hip files, and tests/native/stream_formats_check.cpp compiles it alone under Address + UB sanitizer on the CPU.
//
// A class is a (rate, format) pair: its geometry, its counts and its control words are stream_rates.h's, whatever the format - the
// format only says how the class's samples lie in memory.  What is new is what follows from samples of one and of two bytes sharing
// one block: the byte layout of a tick's frames, the room a bank reserves for it, and what a feed's packets must look like.
#pragma once

#include "stream_rates.h"

// (include/wwhip.h's values: WW_SAMPLE_I16, WW_SAMPLE_MULAW, WW_SAMPLE_ALAW)
#define WW_FMT_I16 0
#define WW_FMT_MULAW 8
#define WW_FMT_ALAW 9

// bytes per sample of a format a class may read; 0: not one (float32 among them)
static inline int format_bytes(int32_t fmt) { return fmt == WW_FMT_I16 ? 2 : (fmt == WW_FMT_MULAW || fmt == WW_FMT_ALAW) ? 1 : 0; }
static inline const char *format_name(int32_t fmt) { return fmt == WW_FMT_I16 ? "int16" : fmt == WW_FMT_MULAW ? "mu-law" : fmt == WW_FMT_ALAW ? "A-law" : "?"; }

struct formats_table {
  int32_t fmt[WW_STREAM_MAX_RATES] = {};  // (all WW_FMT_I16: a bank without formats)
  bool g711 = false;                      // some class reads G.711: the bank's frames and packets are counted in bytes
};

// The next class of a table and its format: rates_add_class where a class is a (rate, format) pair - the same rate may come in two
// formats, the same pair may not come twice; pass = true is the 16 kHz class of the format (int16: the plain pass-through; G.711: a
// decode, still no delay and no history).  1 and "class <k>: <reason>" in `why`, or 0.
static inline int formats_add_class(rates_table &t, formats_table &f, int32_t fmt, bool pass, int32_t rate_in, int32_t rate_out, int64_t up, int64_t down,
                                    int64_t half, int64_t tpp, char *why, size_t cap) {
  const int k = t.K;
  if (k >= WW_STREAM_MAX_RATES) {
    snprintf(why, cap, "class %d: a bank has at most %d rate classes", k, WW_STREAM_MAX_RATES);
    return 1;
  }
  if (!format_bytes(fmt)) {
    snprintf(why, cap, "class %d: format %d: a class reads WW_SAMPLE_I16, WW_SAMPLE_MULAW or WW_SAMPLE_ALAW (float32 streams are not offered)", k, (int)fmt);
    return 1;
  }
  rate_geom g = rates_pass_geom();
  if (!pass) {
    char reason[200];
    if (rate_make_geom(rate_in, rate_out, up, down, half, tpp, g, reason, sizeof reason)) {
      snprintf(why, cap, "class %d: %s", k, reason);
      return 1;
    }
  }
  for (int j = 0; j < k; ++j)
    if (f.fmt[j] == fmt && t.g[j].rate_in == g.rate_in) {
      snprintf(why, cap, "class %d: %d Hz %s is class %d already (two classes of the same input rate and format)", k, g.rate_in, format_name(fmt), j);
      return 1;
    }
  t.g[k] = g;
  t.pass[k] = pass;
  f.fmt[k] = fmt;
  f.g711 = f.g711 || format_bytes(fmt) == 1;
  t.K = k + 1;
  return 0;
}

// Where the next frame starts behind `at` bytes: a G.711 frame at the next byte, an int16 frame at the next even byte
static inline int64_t formats_frame_start(int64_t at, int bytes_per_sample) { return bytes_per_sample == 2 ? (at + 1) & ~(int64_t)1 : at; }

// A tick's frames: ONE byte block, stream s's F(cls[s]) samples of its class's format from byte byte_offs[s]; one pad byte in front
// of an int16 frame that would start on an odd byte, nothing else between the streams.  frame_bytes [S], byte_offs [S + 1] and
// formats [S] may each be nullptr; -> the block's bytes (= byte_offs[S], the end of the last frame).
static inline int64_t formats_layout(const rates_table &t, const formats_table &f, const int32_t *cls, int S, int32_t *frame_bytes, int64_t *byte_offs,
                                     int32_t *formats) {
  int64_t at = 0;
  for (int s = 0; s < S; ++s) {
    const int c = cls[s], b = format_bytes(f.fmt[c]);
    at = formats_frame_start(at, b);
    if (frame_bytes) frame_bytes[s] = t.g[c].F * b;
    if (byte_offs) byte_offs[s] = at;
    if (formats) formats[s] = f.fmt[c];
    at += (int64_t)t.g[c].F * b;
  }
  if (byte_offs) byte_offs[S] = at;
  return at;
}

// the block's bytes at most, whatever the streams move to (every stream in the class of the longest frame, a pad byte in front of
// each): what a bank reserves once
static inline int64_t formats_layout_max(const rates_table &t, const formats_table &f, int S) {
  int64_t m = 0;
  for (int k = 0; k < t.K; ++k) {
    const int64_t b = (int64_t)t.g[k].F * format_bytes(f.fmt[k]);
    m = b > m ? b : m;
  }
  return (int64_t)S * (m + (f.g711 ? 1 : 0));
}

// A feed's packet i of a stream that reads `fmt`: bytes [b0, b1) of the call's data.  1 and the reason in `why` for an int16 packet
// with an odd first byte or an odd length; 0 and its samples in *k otherwise (b1 < b0: a negative count, the caller's refusal).
static inline int formats_packet(int32_t fmt, int i, int64_t b0, int64_t b1, int64_t *k, char *why, size_t cap) {
  if (format_bytes(fmt) == 2) {
    if (b0 & 1) {
      snprintf(why, cap, "packet %d: an int16 packet starts at byte %lld: an odd offset", i, (long long)b0);
      return 1;
    }
    if ((b1 - b0) & 1) {
      snprintf(why, cap, "packet %d: an int16 packet of %lld bytes: an odd length", i, (long long)(b1 - b0));
      return 1;
    }
    *k = (b1 - b0) / 2;
    return 0;
  }
  *k = b1 - b0;
  return 0;
}
