// model_layout.h - what the model loader's packing (model_pack.h, host only) and the kernels that read the packed arrays must
// agree on: the sizes of the operand layouts, each defined here and nowhere else, and the scalar geometry of a loaded model.
// Plain C++: no HIP header, no HIP call.
#pragma once

#include <cstdint>
#include <vector>

// ---- mel filter (fft_device.h, stream_fe.h, frontend.hip) --------------------------------------------------------------------
#define WW_MEL_TAPS 36  // wpad [WW_MEL_TAPS][64]: longest band of the shipped filterbank (checked at model load)
#define MAG_LD 272      // floats per frame of magnitudes in the batch front end: 257 + zero pad to 17 * 16
// Lane form (frontend.hip: LM_MEL_REQ_W, LM_MEL_COMPUTE): the bands, widest first, in three groups of 16 slots; a slot of group g accumulates
// WW_MELV_CAPQ[g] float4 chunks of padded taps (36, 16 and 12 taps), the group's chunks start at chunk WW_MELV_CHUNK0[g].
#define WW_MELV_GROUPS 3
#define WW_MELV_CAPQ {9, 4, 3}
#define WW_MELV_CHUNK0 {0, 9, 13}
#define WW_MELV_CHUNKS 16  // 9 + 4 + 3

// ---- CRNN of the shipped geometry (crnn.hip) ---------------------------------------------------------------------------------
#define CV_KPAD 112  // conv_w, conv_wL, conv_wR [CV_KPAD / 4][32][4]: K = 5 * 20 = 100 in 28 k-quads (the conv loop reads 25)
// split-bf16 planes (crnn_fused_bf16_kernel), each [plane 2 = hi, lo][k-step][tile][lane 64][8]
#define CWB_KS 4    // conv weights, A operand: k-steps of 32 ...
#define CWB_MT 2    // ... and m-tiles of 16 channels
#define WX1B_KS 20  // W_x1, B operand: k-steps of 32 (K = 640) ...
#define WX1B_NT 12  // ... and n-tiles of 16 gate rows (2 * 3H = 192)

// ---- Wavenet, split-bf16 parameter pages (wavenet.hip) -----------------------------------------------------------------------
#define WV_SLOTS 14  // A-operand slots per block: gate (2 k-steps x {sig,tanh} x 2) = 8, res | skip (3 m-tiles x 2) = 6
#define WV_PAGE_U4 (WV_SLOTS * 64)  // one block's parameter page in 16-byte units (the conv biases sit in padded k-slots)

// ---- scalar geometry: filled by the packer, carried by ww_filter_dev / ww_crnn_dev / ww_wave_dev (common.h) -------------------
struct ww_filter_geom {
  int n_mel = 0, n_bins = 0;
  float floor_v = 0, log_off = 0, scale = 0;
  int total_taps = 0, max_len = 0;
  int melv_aligned = 0;  // lane form: every first bin is a multiple of 4
};

struct ww_crnn_geom {
  int n_mel = 0, T = 0, C = 0, KF = 0, KT = 0, SF = 0, ST = 0, PF = 0, PT = 0, OF = 0, OT = 0, H = 0, NOUT = 0, HEAD = 0;
  // Any other conv geometry (utils/CRNN_files/*_old.tflite: 20x5 kernel, stride 8x2, VALID, 74 steps of 96 features)
  // takes the generic kernels of crnn.hip: direct conv, the same MFMA GEMM on K padded to FEATP, step-wise GRUs.
  // So does every recurrent cell but the shipped one (a reset-after GRU of 32 units under a 64-wide head): an LSTM, H = 16, 48, 64 or a
  // head of another width runs rnn_layer_kernel / crnn_head_kernel behind the same conv and GEMM, whatever its conv geometry.
  bool generic = false;
  int FEATP = 0;  // OF*C rounded up to the GEMM's K tile (64)
  int CELL = 0;   // WW_CELL_GRU | WW_CELL_LSTM: G = 3 (z, r, h) or 4 (i, f, c, o) gate blocks of H rows
  int F = 0;      // width of the head's first dense layer, 1..64
  int SEQP = 0;   // 2H rounded up to the GEMM's K tile: row stride of the layer-1 sequence and of wx2 on the layered path
};

struct ww_wave_geom {
  int T = 0, n_mel = 0, C = 0, S = 0, NB = 0, NOUT = 0;
  std::vector<int> dil, order, has_res;
  bool order_is_natural = true;
};

// ---- the geometry plus the device addresses of the arrays: plain pointers, so that host-only code (model_set.h) can translate them
// A loaded model's arrays all lie in ONE device block (ww_model::block), each from a 256-byte boundary, packed on the host by
// model_pack.h; the structs below are model_layout.h's scalar geometry plus the pointers into that block (api.hip: ww_model_load).
struct ww_filter_dev : ww_filter_geom {
  int *start = nullptr;      // [n_mel] first bin of band m
  float *bias = nullptr;
  float *wdense = nullptr;   // [n_mel][n_bins] dense weights (filter.tflite layout)
  float *wpad = nullptr;     // [WW_MEL_TAPS][64] tap-major zero-padded weights of the bands from their first bins (kernel form)
  double *hann = nullptr;    // [512] np.hanning(512) in fp64
  double *tw256 = nullptr;   // [256][2] e^{-2 pi i k / 256}
  double *tw512 = nullptr;   // [256][2] e^{-2 pi i k / 512}
  double *tw16 = nullptr;    // [16 k1][16 j][2] e^{-2 pi i j k1 / 256}
  // Mel filter in lane form for the batched front end (frontend.hip): the bands, sorted by width, are dealt
  // to three groups of 16 "slots"; slot s of group g accumulates one band over 4 * WW_MELV_CAPQ[g] padded taps.
  float *melV = nullptr;     // [WW_MELV_CHUNKS][16 slots] float4: 0.5 * weight of taps 4c..4c+3 (chunks of group 0, 1, 2)
  int *melVmeta = nullptr;   // [3][16]: first bin | band << 16 (band 0xffff: empty slot)
};

struct ww_crnn_dev : ww_crnn_geom {
  float *conv_w = nullptr;   // [CV_KPAD/4][32][4] (MFMA B-operand order); generic: conv_wt
  float *conv_b = nullptr;   // [C]
  float *wx1s = nullptr;     // W_x1 [2*3H][OF*C] (rows: fwd z,r,h then bwd z,r,h) in MFMA B-operand order [OF*C/4][2*3H][4] (crnn_fused_kernel)
  // (G = 3 gate blocks z, r, h of a GRU, 4 blocks i, f, c, o of an LSTM, wherever 3H stands below)
  float *bx1 = nullptr;      // [2*3H]
  float *wh1 = nullptr;      // [2][3H][H]
  float *bh1 = nullptr;      // [2][3H]; zeros for an LSTM (its one bias is bx)
  float *wx2 = nullptr;      // [2*3H][SEQP]: [2*3H][2H] where 2H is a multiple of 64, zero padded behind column 2H otherwise
  float *wx2s = nullptr;     // the same in MFMA B-operand order [2H/4][2*3H][4]
  unsigned short *cwb = nullptr;   // split-bf16 mode: conv weights hi/lo planes in A-operand order (crnn_fused_bf16_kernel)
  unsigned short *wx1b = nullptr;  // split-bf16 mode: W_x1 hi/lo planes in B-operand order
  float *bx2 = nullptr;
  float *wh2 = nullptr;
  float *bh2 = nullptr;
  float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;  // head: w1 [F][2H], b1 [F], w2 [NOUT][F], b2 [NOUT]
  // generic geometry (ww_crnn_geom::generic)
  float *conv_wt = nullptr;    // [KF*KT][C]  (k-major for the implicit GEMM)
  float *conv_wL = nullptr, *conv_wR = nullptr;  // conv_w with the taps that meet a window's zero padding cleared (first 6 / last 7 frames): crnn_rows_kernel
  float *wx1p = nullptr;       // [2*3H][FEATP], zero padded
};

struct ww_wave_dev : ww_wave_geom {
  float *w_in = nullptr, *b_in = nullptr;          // [n_mel][C], [C]
  float *bn_s = nullptr, *bn_t = nullptr;          // [NB][C]
  float *w_gate = nullptr, *b_gate = nullptr;      // [NB][3*C][2C] (cols: sig 0..C-1, tanh C..2C-1), [NB][2C]
  float *w_rs = nullptr, *b_rs = nullptr;          // [NB][C][C+S] (cols: res 0..C-1, skip C..), [NB][C+S]
  float *d_w1 = nullptr, *d_b1 = nullptr, *d_w2 = nullptr, *d_b2 = nullptr;
  uint16_t *wpk = nullptr;                         // split-bf16 parameter pages [NB]{[WV_SLOTS][64][8] bf16 A operands, [7][16] f32 vectors}
};
