// The implicit-GEMM convolution: its launch record, the planner's types, each family's admission predicate and
// launcher, and the fused ResBlock pair.
#pragma once
#include "kernel_base.h"

namespace rvcx {

enum ResMode : int {
  RES_NONE = 0,
  RES_ADD_PRE = 1,   // v = (acc + bias) + R, then alpha, act
  RES_ADD_POST = 2,  // v = act(alpha*(acc + bias)) + R
  RES_RSUB_POST = 3, // v = R - act(alpha*(acc + bias))
};

enum AccMode : int {
  ACC_STORE = 0,   // y = v
  ACC_ADD = 1,     // y = y + v
  ACC_ADD_DIV = 2, // y = (y + v) / acc_div
};

enum OutMap : int {
  OUT_ROWS = 0,       // y[b][m][n]
  OUT_UPSAMPLE2D = 1, // 2-D ConvTranspose phase scatter: n = (ph*2+pw)*Cv + co -> pixel (2h+ph, 2w+pw)
};

// WSPLIT_S2D: the few-channel 3x3 convs' fp16 image (conv2d_small.hip k_s2d_wsplit: fragment-major, no column padding)
enum WsplitFmt : int { WSPLIT_BF16 = 0, WSPLIT_H16 = 1, WSPLIT_S2D = 2 };

// Implicit-GEMM convolution:  y[b][m][n] = epi( sum_tap sum_c pre(X[b][row(m,tap)][c]) * W[tap][n][c] )
struct ConvArgs {
  // A operand (activations)
  const float* x = nullptr;
  long long x_bs = 0;   // batch stride (floats)
  int ldx = 0;          // row stride
  int T_in = 0;         // valid input rows (1-D) ; for 2-D: H_in
  int W_in = 0;         // 2-D: input width
  int C_in = 0;         // contraction channels per tap
  int pre_act = ACT_NONE;
  float pre_slope = 0.f;
  const float* pre_mask = nullptr;  // [b][row] multiplier applied to input rows (1-D only)
  long long pre_mask_bs = 0;
  // B operand (weights): w + tap*w_ts + n*ldw + c
  const float* w = nullptr;
  long long w_bs = 0;
  long long w_ts = 0;
  int ldw = 0;
  // geometry
  int taps = 1;
  int stride = 1, dil = 1, pad = 0;     // 1-D
  int KH = 1, KW = 1, padh = 0, padw = 0; // 2-D (taps = KH*KW; tap = kh*KW + kw)
  // output
  float* y = nullptr;
  long long y_bs = 0;
  int ldy = 0;
  int T_out = 0;   // output rows (1-D) ; 2-D: H_out (tile grid), W_out
  int W_out = 0;
  int N = 0;
  int out_map = OUT_ROWS;
  int out_cv = 0;  // OUT_UPSAMPLE2D: real output channels
  // epilogue
  const float* bias = nullptr;
  long long bias_bs = 0;
  float alpha = 1.f;
  int act = ACT_NONE;
  float slope = 0.f;
  const float* res = nullptr;
  long long res_bs = 0;
  int ldr = 0;
  int res_mode = RES_NONE;
  const float* mask = nullptr;  // [b][m] output-row multiplier (applied last, after acc_mode)
  long long mask_bs = 0;
  int acc_mode = ACC_STORE;
  float acc_div = 1.f;
  // WaveNet gate (commons.py:88-103) in the split-K combine: N = 2 gate_h columns; y[m][c] (c < gate_h) =
  // tanh(v[c] + g[c]) * sigmoid(v[c + gate_h] + g[c + gate_h]), v = acc + bias, g = gate_g + b * gate_g_bs. Forces a
  // split (ksplit >= 2); no other epilogue field may be set.
  int gate_h = 0;
  const float* gate_g = nullptr;
  long long gate_g_bs = 0;
  // post-norm LayerNorm in the split-K combine (a Transformer block's residual + norm, attentions.py:221-231 with
  // norm_layers_2, modeling_hubert.py final_layer_norm): y[m] = LN(res[m] + v[m]) * ln_g + ln_b over the N columns, v the
  // epilogue value (bias, alpha, act, mask) with res_mode RES_NONE (res / ldr / res_bs name the LN's residual input).
  // Forces a split (ksplit >= 2); 1-D, batch_inner 1, N <= 1024. Equals the two passes to fp32 rounding of the row sums.
  const float* ln_g = nullptr;
  const float* ln_b = nullptr;
  float ln_eps = 1e-5f;
  // grid z = batch * batch_inner; pointer offset = zo * *_bs + zi * *_bs2 (mask: zo only)
  int batch = 1;
  int batch_inner = 1;
  long long x_bs2 = 0, w_bs2 = 0, y_bs2 = 0, res_bs2 = 0, bias_bs2 = 0;
  int math = 0;   // contraction arithmetic: 0 = default (RVCX_CONV_MATH), 1 = native fp32 MFMA, 2 = fp32 via 3 bf16 planes
  int w_static = 0;             // the B operand is a constant weight tensor (callers set it; enables the cache)
  // the pre-split weight image of the streamed kernels, in the format the plan names (ConvPlan::wsplit_fmt): the
  // runtime's cache for static weights, or the caller's own
  const void* wsplit = nullptr;  // ((chunk * taps + tap) * wsplit_npad + n) rows of [hi|mid|lo] x 32 bf16
  // read by the kernels from their kernarg copy; written by conv_run alone, from the plan. ws (the caller's allocation
  // of ConvPlan::slab_floats) holds ksplit partial [rows][N] tiles per batch entry
  int wsplit_npad = 0;
  int wsplit_fmt = 0;  // WSPLIT_BF16: three bf16 planes (every streamed kernel); WSPLIT_H16: two fp16 planes + scale tail
                       // (conv_wsb16_kernel only: the two-plane fp16 arithmetic and the reduced-precision mode)
  int ksplit = 1;
  int no_splitk = 0;
  // rows the dispatcher plans for (1-D; 0 = T_out): the kernel family, the tile and ksplit are chosen as for a launch
  // of plan_T rows, so a launch over a window of a longer sequence (the decoder's output window, runtime_synth.cpp)
  // gets the arithmetic of the full-length launch. Grids, workspaces and slabs are sized by T_out.
  int plan_T = 0;
  // opt-in reduced precision (the generator's weight-streamed convs of a realtime hop, rvcx_rt_opts::gen_precision):
  // fp16 operands (the WSPLIT_H16 image's hi plane), one MFMA product per step. Never set on the parity path.
  int lowp = 0;
  long long ws_rows = 0;
  float* ws = nullptr;
  // + the NSF noise conv of this output (hifigan_nsf.py:196-199: x = ups(x) + noise_convs(har)), fused into the
  // epilogue of the polyphase ConvTranspose (1-D, unsplit, store_tile16 kernels, plain bias epilogue; one tap,
  // nz_kk = 1, the only length the dispatcher admits): output row m,
  // column n = p * nz_C + c (phase p of nz_u) gets nz_b[c] + sum_q w(q, c) har[(m nz_u + p) nz_stride + q], q < nz_kk,
  // with w(q, c) = nz_w[((q / nz_stride) nz_C + c) nz_stride + q % nz_stride] (k_noise_add's layout and fma order)
  const float* nz_har = nullptr;
  long long nz_bs = 0;
  int nz_stride = 0, nz_kk = 0, nz_u = 1, nz_C = 0;
  const float* nz_w = nullptr;
  const float* nz_b = nullptr;
  // extra dynamic LDS per workgroup (bytes): fewer of this launch's workgroups fit a CU beside the critical stream's
  // (an occupancy throttle for off-critical-path work; the gather-streamed and LDS-staged kernels honour it)
  int lds_pad = 0;
  // 2-D, images of different heights in one batch (device array indexed by the outer batch entry, each <= T_in): image
  // b has h_in[b] valid rows and a tap at a row from h_in[b] on reads zero, whatever the buffer holds there -- the
  // padding a launch on that image alone has at its last row. Its output rows from h_in[b] on are written and hold no
  // meaning. The planner does not read it: the route is the equal-height batch's (conv_run refuses a family without
  // it). Last in the record: no other field's place in the kernels' argument copy moves.
  const int* h_in = nullptr;
};

// the kernel families (the plan's, and the kernel-timing records' of rvcx_profile). CK_WSB is retired: no plan names
// it; the slot stays so the recorded numbers of the other families do not move
enum ConvKind : int { CK_WSB16 = 0, CK_WSB, CK_GS, CK_GSW, CK_RBPAIR, CK_SMALL2D, CK_EMU, CK_GEMM, CK_TINY, CK_WST,
                      CK_OTHER, CK_COUNT };
const char* conv_kind_name(int k);
// Tile ids, by the numbers DESIGN.md, profiles/ and bench_conv's command line know them by. Every tile that exists is
// listed: the LDS-staged kernels' native fp32 tiles 1 and 3 (conv_gemm.hip) and bf16-split tiles 12 and 13
// (conv_emu.hip) -- the other ids below 20 named tiles the planner never chose and are gone --, the
// weight-streamed 23..27 (conv_wsb.hip), the gather-streamed 30 (conv_gs.hip)
enum ConvTile : int {
  TILE_NONE = -1,  // the family has one form (tiny, 3x3 small-channel, weight-stationary)
  TILE_F32_128x32 = 1, TILE_F32_64x64 = 3, TILE_EMU_128x32 = 12, TILE_EMU_64x64 = 13,
  TILE_WSB_128x64 = 23, TILE_WSB_256x32 = 24, TILE_WSB_128x128 = 25, TILE_WSB_128x64_1x4 = 27, TILE_GS_64x64 = 30,
};
// a numerics test's or a benchmark's override of the policy: the family (a ConvKind, -1 = the policy's), its tile
// (-1 = the policy's for that family) and the GEMM pipeline (0 = the policy: on for plain GEMMs, < 0 off, > 0 on)
struct ConvForce {
  int kind = -1, tile = TILE_NONE, pipe = 0;
};
// What one launch runs: the family, its tile, the split over K with the floats of slab it needs (ConvArgs::ws), the
// weight image the family reads (a WsplitFmt, -1 = none) and whether the runtime's cache is to supply it
// (needs_image), and the LDS-staged families' GEMM-pipeline form. kind CK_OTHER: no family admits the form.
struct ConvPlan {
  ConvKind kind;
  int tile, ksplit;
  long long slab_floats;
  int wsplit_fmt;
  bool needs_image, pipe;
};
// The one place a contraction's route is decided (conv_dispatch.hip). Pure host code: it reads the record's form --
// shape, strides, epilogue fields, arithmetic -- and its pointers for nullness and alignment only; no field conv_run
// writes. static_weight: the B operand is a constant tensor (only those take the streamed kernels).
ConvPlan conv_plan(const ConvArgs& a, bool two_d, bool static_weight, const ConvForce& force = ConvForce());
// launch the plan: that family's launcher and, for a split, the combine. a.ws holds plan.slab_floats floats when
// plan.ksplit > 1, a.wsplit the image when plan.wsplit_fmt >= 0. A launcher that refuses is an error
// (hipErrorInvalidValue), never another family; forced: not even another tile of the LDS-staged families
hipError_t conv_run(const ConvPlan& plan, const ConvArgs& a, bool two_d, hipStream_t s, bool forced = false);
// the contraction arithmetic a launch gets: ConvArgs::math, else RVCX_CONV_MATH (1 fp32 MFMA, 2 bf16 split, 3 fp16 split)
int conv_math(int requested);

// The admission predicates (*_eligible, *_fits) are questions about the caller's form alone: admitted means that
// family's launcher takes the launch.

// 3x3/pad-1 2-D convs with C_in, N in {16, 32} on 16x16x4 MFMA fragments (conv2d_small.hip); the planner routes
// the shapes conv2d_small_fits accepts there
bool conv2d_small_fits(const ConvArgs& a);
hipError_t conv2d_small(const ConvArgs& a, hipStream_t s);
// their WSPLIT_S2D image (the fp16-split form reads it; built by conv_wsplit_build for that format)
long long small2d_wsplit_bytes(const ConvArgs& a);
hipError_t small2d_wsplit_build(const ConvArgs& a, void* out, hipStream_t s);

// weight-streamed split conv (conv_wsb.hip): eligibility (1-D, stride 1, C_in % 32 == 0, halo <= 64 rows), the
// pre-split weight image and its launch
bool conv_wsb_eligible(const ConvArgs& a, bool two_d = false);
bool conv_wsb_tile(int cfg, int& BM, int& BN);  // cfg 23, 24, 25, 27 -> tile
int conv_wsplit_npad(int N);
long long conv_wsplit_bytes(const ConvArgs& a);
hipError_t conv_wsplit_build(const ConvArgs& a, void* out, hipStream_t s);
hipError_t conv_wsb_launch(const ConvArgs& a, int cfg, hipStream_t s, bool two_d = false,
                           int ksplit = 1);

// gather-streamed split conv (conv_gs.hip) for the short contractions: pre-split weights (the conv_wsb image) in a
// register ring, A gathered per (chunk, tap) step; 1-D (any stride / dilation) and 2-D (stride 1, OUT_ROWS), C_in % 32
// == 0, split-K capable. cfg 30 -> its 64 x 64 tile
bool conv_gs_eligible(const ConvArgs& a, bool two_d);
bool conv_gs_form(const ConvArgs& a, bool two_d);  // eligible but for ConvArgs::lowp (these kernels have no such mode)
bool conv_gsw_eligible(const ConvArgs& a);  // the windowed 2-D form (split-K slices of whole 32-channel chunks)
hipError_t conv_gs_launch(const ConvArgs& a, int cfg, hipStream_t s, bool two_d, int ksplit);

// weight-stationary form of the fp16-split conv (conv_wst.hip) for the short 64 / 128-channel convs (k = 3 ResBlock
// convs, ConvTranspose phases): 1-D, C_in = N in {64, 128}, 2-3 taps, halo <= 16, no or leaky-ReLU pre-activation,
// the WSPLIT_H16 image, unsplit, bias / leaky-ReLU / RES_ADD_POST / acc modes / the fused noise conv; bit-identical to
// conv_wsb16_kernel. The planner takes it ahead of the weight-streamed tiles
bool conv_wst_fits(const ConvArgs& a, bool two_d);
hipError_t conv_wst_launch(const ConvArgs& a, hipStream_t s);

// fused ResBlock dilation pair (resblock_fused.hip): y (acc_mode) <- conv2(lrelu(conv1_d(lrelu(x)) + b1)) + b2 + x,
// x / y [B][T][C] (x != y), C in {32, 64}, odd k, (k - 1) / 2 * d <= 30; w1s / w2s are rb_wsplit_build images
// of [k][C][C] fp32 weights
struct RbPairArgs {
  const float* x = nullptr;
  long long x_bs = 0;
  const void* w1s = nullptr;
  const float* b1 = nullptr;
  const void* w2s = nullptr;
  const float* b2 = nullptr;
  int C = 0, k = 0, d = 1, T = 0, B = 1;
  float* y = nullptr;
  long long y_bs = 0;
  int acc_mode = ACC_STORE;
  float acc_div = 1.f;
  int wfmt = 0;   // RB_WBF16: w1s / w2s are three-plane bf16 images (the exact split); RB_WF16: two-plane fp16 images
  int lowp = 0;   // opt-in reduced precision (rvcx_rt_opts::gen_precision): the fp16 images' hi planes alone
};
enum RbWfmt : int { RB_WBF16 = 0, RB_WF16 = 1 };
bool rb_pair_fits(int C, int k, int d);
long long rb_wsplit_bytes(int C, int k, int wfmt = RB_WBF16);
hipError_t rb_wsplit_build(const float* w, int C, int k, void* out, hipStream_t s, int wfmt = RB_WBF16);
hipError_t rb_pair(const RbPairArgs& a, int cfg, hipStream_t s);

}  // namespace rvcx
