// The conv dispatcher: which kernel family and tile a contraction gets (pick_*, conv_wsb_route), when it is split over
// K (conv_plan_splitk), and conv1d / conv2d, which try the families in order. Every policy number below carries the
// measurement that set it.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "conv_common.h"

namespace rvcx {

constexpr int CK = 32;  // contraction channels per (chunk, tap) step of every MFMA conv kernel

namespace {

// Tile per shape class, measured on MI355X (same-box A/B of the whole pipeline, bench.py at each policy):
// one 32x32 accumulator per wave with 4 waves per block beats the larger per-wave tiles in the pipeline:
// 128x32 for N <= 32 and for the long-tap 1-D convs (the generator's dilated ResBlock convs), 64x64
// otherwise; split-K when the output grid cannot fill 256 CUs.
inline int env_cfg(const char* name, int dflt) {
  const char* e = rvcx_knob(name);
  return e ? std::atoi(e) : dflt;
}
// contraction arithmetic: 1 = native fp32 MFMA (conv_gemm_kernel), 2 = fp32 through the 3-way bf16 split everywhere
// (conv_emu.hip), 3 (the default) = as 2 except the weight-streamed kernel and the fused ResBlock pairs (the generator),
// which take the two-plane fp16 split (the WSPLIT_H16 / RB_WF16 images: three MFMA products per step instead of six,
// measured as accurate as native fp32, bench_conv / tests/test_gpu_conv_math.py); ConvArgs::math overrides
// RVCX_CONV_MATH (f32 | split | h16)
inline int conv_math(const ConvArgs& a) {
  static const int env = [] {
    const char* e = rvcx_knob("RVCX_CONV_MATH");
    if (e && (std::string(e) == "f32" || std::string(e) == "1")) return 1;
    if (e && (std::string(e) == "split" || std::string(e) == "2")) return 2;
    return 3;
  }();
  return a.math > 0 ? a.math : env;
}

// Tile per shape class in split mode, from build/bench_conv on MI355X (TF/s, split vs the native fp32 kernel):
// long-tap convs 128x32 (C128 k11 155 vs 114, C256 k11 138 vs 106), short taps and GEMMs 64x64 (C128 k3 + residual
// 101 vs 78, HuBERT qkv 52 vs 38), narrow short convs (N <= 32, taps < 5: the 32-channel ResBlock k=3, latency
// bound) stay on the native kernel (53 vs 47): both arithmetics are fp32 accurate, so the choice is per shape. The
// U-Net's 3x3 convs: 64x64 (C2 26.7 -> 25.9 ms vs 128x64)
template <bool TWO_D>
int pick_emu(const ConvArgs& a) {
  if (TWO_D) return a.N <= 32 ? 12 : 13;
  if (a.N <= 32) return a.taps >= 5 ? 12 : 1;
  if (a.taps >= 5) return 12;
  return 13;
}

template <bool TWO_D>
int pick_cfg(const ConvArgs& a) {
  if (a.force_cfg >= 0) return a.force_cfg;
  if (conv_math(a) >= 2) return pick_emu<TWO_D>(a);
  // N <= 32 and the 1-D convs with taps >= 5 (A/B: 32.8 vs 33.6 ms): 128 x 32; everything else 64 x 64
  if (a.N <= 32) return 1;
  if (!TWO_D && a.taps >= 5) return 1;
  return 3;
}

inline void cfg_tile(int cfg, int& BM, int& BN) {
  if (conv_emu_tile(cfg, BM, BN)) return;
  static const int t[10][2] = {{256, 32}, {128, 32}, {128, 64}, {64, 64}, {128, 128}, {64, 128}, {256, 64},
                               {64, 64}, {128, 32}, {128, 128}};
  BM = t[cfg][0];
  BN = t[cfg][1];
}

// the rows every policy decision below is made for: ConvArgs::plan_T where the caller launches a window of a longer
// sequence and wants the full-length launch's kernel, tile and ksplit (1-D only), else the launch's own rows
inline int plan_rows(const ConvArgs& a) { return (a.plan_T > 0 && a.W_out <= 0) ? a.plan_T : a.T_out; }

// weight-streamed split kernel (conv_wsb.hip) tiles: 256x32 for N <= 32, else 128x64 (2 x 2 waves of 64 x 32;
// RVCX_WCFG_* override). bench_conv on MI355X with the register epilogue (TF/s, vs the LDS-staged split kernel's
// best tile): C256 k11 174 vs 142, C128 k11 204 vs 160, C128 k7 185 vs 144, C128 k3 124 vs 118, ConvTranspose
// phases 105 / 124 / 94 vs 95 / 117 / 96; the 32-channel convs lose (C32 k11 95 vs 115).
// Round 3: the same tiles on v_mfma_f32_16x16x32_bf16 (cfg 24 / 23) hold a higher clock under the power-limited load
// (bench_conv r03h, same box, 32x32x16 -> 16x16x32 TF/s: C128 k11 198 -> 214, k7 181 -> 194, k3 124 -> 131, C256 k11
// 171 -> 182, C64 k11 177 -> 190, ConvTranspose phases 108 / 125 / 94 -> 114 / 129 / 99).
// Round 3, wave layout per shape (cfg 23 = 2 x 2 waves of 64 x 32, 27 = 1 x 4 waves of 128 x 16, 28 = 256 x 64 as
// 2 x 2 waves of 128 x 32). bench_conv r03bc (warm, TF/s): short taps (k = 3 ResBlock convs, ConvTranspose phases)
// gain on 27 (C128 k3+res 141 -> 159, C64 k3+res 90 -> 109, up3 152 -> 159: a wave's 3 B loads per step feed 8 row
// blocks), k = 7 / 11 at C_in <= 128 a little on 28 (C128 k11 244 -> 252), C256 k11 loses on 28 (208 -> 171). In the
// C2 step (rocprof r03ab, weight-streamed time per step): 27 for k <= 3 7969 -> 7919 us, 28 for k = 7 / 11 +147 us
// (cold activations, 2 workgroups per CU), so the long convs stay on 23 (RVCX_WCFG_LONG=28 to compare)
// Round 6: the 128-channel k = 7 / 11 convs on 128 x 128 tiles (cfg 25, 2 x 2 waves of 64 x 64: C128 k11 402 vs 380
// TF, k7 346 vs 340 in bench_conv r06a; same-box C2 12.91 / 12.99 vs 13.04 / 13.01 ms, r06b); at 256 input channels
// (C256 k11 288 vs 330) and 64 output channels (half of each tile idle) cfg 23 stays. RVCX_WCFG_LONG forces one tile
// for every long conv (A/B aid)
inline int pick_wsb(const ConvArgs& a) {
  static const int c_long = env_cfg("RVCX_WCFG_LONG", 0);
  if (a.wsb == 2) return 30;  // gather-streamed (conv_gs.hip): the short contractions
  if (a.N <= 32) return 24;
  // the wide ConvTranspose phase group of the second upsample (18600 rows x 1280 columns, 2 taps) on 128 x 128 tiles:
  // bench_conv r06a h25 254.6 vs h27 232.2 TF (the first one, 1550 rows x 3072, loses there: 189 vs 206)
  if (a.taps <= 3 && a.N >= 1024 && plan_rows(a) >= 8192 && a.C_in < 512 && c_long == 0) return 25;
  if (a.taps <= 3) return 27;
  if (c_long > 0) return c_long;
  return (a.C_in < 256 && a.N >= 128) ? 25 : 23;
}
}  // namespace
int conv_wsb_pick(const ConvArgs& a) {
  ConvArgs b = a;
  b.wsb = 1;
  return pick_wsb(b);
}
thread_local int g_conv_kind = CK_OTHER;
int conv_last_kind() { return g_conv_kind; }
const char* conv_kind_name(int k) {
  static const char* const names[CK_COUNT] = {"conv_wsb16_kernel", "conv_wsb_kernel", "conv_gs16_kernel",
                                              "conv_gsw16_kernel", "k_rb_pair", "k_conv2d_h16/k_conv2d_small",
                                              "conv_emu_kernel", "conv_gemm_kernel", "conv_tiny_kernel",
                                              "conv_wst16_kernel", "other"};
  return (k >= 0 && k < CK_COUNT) ? names[k] : "other";
}

namespace {

template <bool TWO_D>
hipError_t dispatch(const ConvArgs& a_in, hipStream_t s) {
  const ConvArgs& a = a_in;
  if (a.N <= 0 || a.T_out <= 0 || a.batch <= 0) return hipSuccess;
  if (a.C_in <= 0 || a.taps <= 0) return hipErrorInvalidValue;
  // the fused noise conv lives in the 16x16 tile stores' unsplit epilogue only (the caller routes it to such a kernel)
  const bool nz = a.nz_har != nullptr;
  if (nz && (TWO_D || (a.ws && a.ksplit > 1) || a.nz_C <= 0 || a.nz_stride <= 0 ||
             a.nz_kk != 1 ||
             a.N != a.nz_u * a.nz_C || a.out_map != OUT_ROWS))
    return hipErrorInvalidValue;
  // the gate and the LayerNorm are applied by the combine
  if ((a.gate_h > 0 || a.ln_g) && !(a.ws && a.ksplit > 1)) return hipErrorInvalidValue;
  if (tiny_fits(a)) {
    if (nz) return hipErrorInvalidValue;
    g_conv_kind = CK_TINY;
    return launch_tiny(a, TWO_D, s);
  }
  if (!nz && !(a.ws && a.ksplit > 1) && rows1x1_fits(a, TWO_D)) {
    g_conv_kind = CK_TINY;
    return launch_rows1x1(a, TWO_D, s);
  }
  if (a.wsb == 2 && a.wsplit && conv_math(a) >= 2 && conv_gs_eligible(a, TWO_D)) {
    const int ks = (a.ws && a.ksplit > 1) ? a.ksplit : 1;
    const int cfg = a.force_cfg >= 30 ? a.force_cfg : pick_wsb(a);
    g_conv_kind = (TWO_D && cfg == 30 && conv_gsw_eligible(a)) ? CK_GSW : CK_GS;
    hipError_t e = conv_gs_launch(a, cfg, s, TWO_D, ks);
    if (e == hipSuccess && ks > 1) e = launch_splitk_reduce(a, ks, TWO_D, s);
    if (e != hipErrorInvalidValue) return e;
  }
  if (a.wsb == 1 && a.wsplit && conv_math(a) >= 2 && conv_wsb_eligible(a, TWO_D)) {
    const int ks = (a.ws && a.ksplit > 1) ? a.ksplit : 1;
    // the short 64 / 128-channel convs on the weight-stationary kernel (conv_wst.hip; force_cfg 20..39 keeps a
    // weight-streamed tile for comparisons)
    if (ks == 1 && (a.force_cfg < 20 || a.force_cfg == 40) && conv_wst_fits(a, TWO_D)) {
      g_conv_kind = CK_WST;
      hipError_t e = conv_wst_launch(a, s);
      if (e != hipErrorInvalidValue) return e;
    }
    const int cfg = a.force_cfg >= 20 && a.force_cfg < 40 ? a.force_cfg : pick_wsb(a);
    g_conv_kind = CK_WSB16;
    hipError_t e = conv_wsb_launch(a, cfg, s, TWO_D, ks);
    if (e == hipSuccess && ks > 1) e = launch_splitk_reduce(a, ks, TWO_D, s);
    if (e != hipErrorInvalidValue) return e;
  }
  if (nz) return hipErrorInvalidValue;  // no kernel with a 16x16 tile store took it
  // 3x3 convs with 16/32 channels: 16x16x4 MFMA fragments (conv2d_small.hip)
  if (TWO_D && a.force_cfg < 0 && conv2d_small_fits(a)) {
    g_conv_kind = CK_SMALL2D;
    return conv2d_small(a, s);
  }
  const int cfg = pick_cfg<TWO_D>(a);
  const bool emu = cfg >= 10;  // the arithmetic: fp32 through bf16 planes (conv_emu.hip) or native fp32 (conv_gemm.hip)
  g_conv_kind = emu ? CK_EMU : CK_GEMM;
  // plain GEMMs (1-D, one tap, stride 1) take the double-buffered pipeline unless a.pipe < 0; a.pipe > 0 forces it
  // (benchmarks)
  const bool gemm = !TWO_D && a.taps == 1 && a.stride == 1;
  const bool pipe = gemm && a.pipe >= 0;
  const int ksplit = (a.ws && a.ksplit > 1) ? a.ksplit : 1;
  auto run = [&](int c, bool p) -> hipError_t {
    hipError_t e = emu ? conv_emu_launch(a, c, TWO_D, p, ksplit, s) : conv_gemm_launch(a, c, TWO_D, p, ksplit, s);
    if (e != hipSuccess || ksplit == 1) return e;
    return launch_splitk_reduce(a, ksplit, TWO_D, s);
  };
  hipError_t e = run(cfg, pipe);
  if (e == hipErrorInvalidValue && pipe) e = run(cfg, false);  // tile without a GEMM-pipeline instantiation
  if (e == hipErrorInvalidValue && a.force_cfg < 0) {
    // the tile's halo does not fit in LDS (long strided taps) or the shape class has no such instantiation: the two
    // fallback tiles of that arithmetic, 64 x 64 then 128 x 32
    for (int alt : {emu ? 13 : 3, emu ? 12 : 1}) {
      if (alt == cfg) continue;
      e = run(alt, false);
      if (e != hipErrorInvalidValue) break;
    }
  }
  return e;
}

}  // namespace

long long conv_plan_splitk(ConvArgs& a, bool two_d) {
  a.ksplit = 1;
  if (a.N <= 0 || a.T_out <= 0 || a.no_splitk) return 0;
  if (tiny_fits(a)) return 0;
  if (two_d && a.force_cfg < 0 && conv2d_small_fits(a)) return 0;
  int BM, BN;
  if (a.wsb == 2) {  // the gather-streamed tile
    conv_gs_tile(a.force_cfg >= 30 ? a.force_cfg : pick_wsb(a), BM, BN);
  } else if (a.wsb) {  // the weight-streamed tile (pick_wsb)
    if (!conv_wsb_tile(a.force_cfg >= 20 ? a.force_cfg : pick_wsb(a), BM, BN)) return 0;
  } else {
    cfg_tile(two_d ? pick_cfg<true>(a) : pick_cfg<false>(a), BM, BN);
  }
  // the decisions (whether to split, ksplit) are made for plan_rows(a) rows, the slab for the launch's own T_out
  const int T_plan = two_d ? a.T_out : plan_rows(a);
  long long mtiles, mtiles_real;
  if (!two_d) {
    mtiles = (T_plan + BM - 1) / BM;
    mtiles_real = (a.T_out + BM - 1) / BM;
  } else {
    const int rw = a.W_out < BM ? a.W_out : BM;
    const int rh = BM / rw;
    mtiles = mtiles_real = (long long)((a.T_out + rh - 1) / rh) * ((a.W_out + rw - 1) / rw);
  }
  const long long tiles = mtiles * ((a.N + BN - 1) / BN) * a.batch * a.batch_inner;
  const long long tiles_real = mtiles_real * ((a.N + BN - 1) / BN) * a.batch * a.batch_inner;
  const int iters = ((a.C_in + CK - 1) / CK) * a.taps;
  const double M = two_d ? (double)a.T_out * a.W_out : (double)T_plan;
  const double flops = 2.0 * M * a.N * (double)a.C_in * a.taps * a.batch * a.batch_inner;
  // split only where the output grid leaves CUs idle AND the contraction is long enough to pay
  // for the extra combine launch (~5-10 us): a tile's (chunk, tap) steps are a serial chain of
  // ~1.5-2 us each (global B load -> LDS -> barrier -> MFMA), so a handful of tiles walking >= 16 steps
  // is latency-bound whatever the FLOP count (RMVPE's deepest levels at streaming sizes: 8 tiles x 144
  // steps = 264 us unsplit)
  // same-box A/B of C2 (round 2, with the 32-bit combine): (target, tiles, min_iters) = (512, 192, 4) 22.59 ms,
  // (768, 384, 8) 22.82, (512, 256, 4) 22.70, (384, 256, 4) 22.64, (1024, 384, 8) 23.33
  static const int target = env_cfg("RVCX_SPLITK_TARGET", 512);  // workgroups a split launch aims for
  constexpr int min_tiles = 192;  // grids with at least this many tiles stay unsplit
  constexpr int min_iters = 4;    // shortest contraction worth a split
  // a gated WaveNet in_layer always splits: its gate lives in the combine (ConvArgs::gate_h)
  const bool combine_epi = a.gate_h > 0 || a.ln_g;  // an epilogue only the combine applies: always split
  if (!combine_epi && (tiles >= min_tiles || iters < min_iters || (flops < 1.0e8 && iters < 16))) return 0;
  int ks = (int)((target + tiles - 1) / tiles);
  // the gather-streamed kernels keep >= 8 (chunk, tap) steps per slice: below that a slice is all prologue and
  // epilogue and the extra slab + combine launch cost more than the parallelism gains (bench_gs r03s, cold: HuBERT
  // 768 -> 768 ks 1 22.1 us vs ks 4 27.6, TextEncoder 1x1 ks 1 11.6 vs ks 3 14.4, U-Net 196 px ks 8 19.8 vs ks 16
  // 21.8, 3136 px ks 2 20.2 vs ks 6 27.3; the 3072 -> 768 linear keeps ks 4: 48.6 vs 62.8 unsplit)
  constexpr int gs_min_steps = 8;  // same-box C2: 2 17.73, 8 17.72, 16 17.86, 24 17.97 ms
  ks = std::min(ks, a.wsb == 2 ? iters / gs_min_steps : iters / 2);
  ks = std::min(ks, 32);
  // the windowed 2-D gather-streamed kernel splits by whole 32-channel chunks (bench_gs: U-Net 784 px ks 8 and 3136 px
  // ks 4 beat the 10 and 6 the step count would give)
  if (a.wsb == 2 && two_d && (a.force_cfg < 0 || a.force_cfg == 30) && conv_gsw_eligible(a))
    ks = std::min(ks, (a.C_in + CK - 1) / CK);
  if (combine_epi && iters >= 2) ks = std::max(ks, 2);
  if (ks < 2) return 0;
  a.ksplit = ks;
  a.ws_rows = two_d ? (long long)a.T_out * a.W_out : a.T_out;
  return std::max((long long)ks * a.ws_rows * a.N * a.batch * a.batch_inner, tiles_real * ks * BM * BN);
}

bool conv_wsb_wants(const ConvArgs& a) {
  if (conv_math(a) < 2 || !conv_wsb_eligible(a)) return false;
  // where it measured faster (bench_conv, profiles/r02i_bench_conv.txt: 128 x 64 tiles of 2 x 2 waves of 64 x 32
  // with the register epilogue; C2 A/B): N >= 64 with >= 2 taps (ResBlock convs at 64-256 channels incl. k = 3, the
  // polyphase ConvTranspose phases; the 64-channel stage on 128x64 tiles beat the fused pair), on a grid that fills
  // the chip
  constexpr int min_taps = 2, min_tiles = 512, min_n = 64;
  if (a.N < min_n || a.taps < min_taps) return false;
  const long long tiles = (long long)((plan_rows(a) + 127) / 128) * ((a.N + 63) / 64) * a.batch;
  return tiles >= min_tiles;
}

int conv_wsb_route(const ConvArgs& a, bool two_d) {
  if (conv_math(a) < 2 || tiny_fits(a)) return 0;
  if (two_d && conv2d_small_fits(a)) return 0;
  // the weight-streamed kernel on small grids (split-K) and on the U-Net's 3x3 convs measured slower than the
  // gather-streamed one (HuBERT / TextEncoder GEMMs +0.7 ms, U-Net +0.8 ms: with few M tiles every wave re-streams its
  // B fragments from L2)
  if (!two_d && conv_wsb_wants(a)) return 1;
  // everything else with a static weight, 32-channel chunks and >= 64 outputs: the short contractions
  if (a.N >= 64 && conv_gs_eligible(a, two_d)) return 2;
  return 0;
}

int conv_math_of(const ConvArgs& a) { return conv_math(a); }
int conv_unstreamed_kind(const ConvArgs& a) {
  if (tiny_fits(a) || (!(a.ws && a.ksplit > 1) && rows1x1_fits(a, false))) return CK_TINY;
  return pick_cfg<false>(a) >= 10 ? CK_EMU : CK_GEMM;
}
hipError_t conv1d(const ConvArgs& a, hipStream_t s) { return dispatch<false>(a, s); }
hipError_t conv2d(const ConvArgs& a, hipStream_t s) { return dispatch<true>(a, s); }

}  // namespace rvcx
