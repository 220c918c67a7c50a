// model_layout.h - what the model loader's packing (model_pack.h, host only) and the kernels that read the packed arrays must
// agree on: the sizes of the operand layouts, each defined here and nowhere else, and the scalar geometry of a loaded model.
// Plain C++: no HIP header, no HIP call.
#pragma once

#include <vector>

// ---- mel filter (fft_device.h, stream_fe.h, frontend.hip) --------------------------------------------------------------------
#define WW_MEL_TAPS 36  // wpad [WW_MEL_TAPS][64]: longest band of the shipped filterbank (checked at model load)
#define MAG_LD 272      // floats per frame of magnitudes in the batch front end: 257 + zero pad to 17 * 16
// Lane form (frontend.hip: LM_MEL_TILE): the bands, widest first, in three groups of 16 slots; a slot of group g accumulates
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
  bool generic = false;
  int FEATP = 0;  // OF*C rounded up to the GEMM's K tile (64)
};

struct ww_wave_geom {
  int T = 0, n_mel = 0, C = 0, S = 0, NB = 0, NOUT = 0;
  std::vector<int> dil, order, has_res;
  bool order_is_natural = true;
};
