// The conv dispatcher. conv_plan decides, once and on the host alone, which kernel family and tile a contraction gets,
// whether it is split over K and which weight image it reads; conv_run launches exactly that plan. Every policy number
// below carries the measurement that set it.
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
// otherwise; split-K when the output grid cannot fill 256 CUs. Those two shapes are the LDS-staged tiles that exist
// (ConvTile); the larger ones they beat are gone, their bench_conv tables kept (DESIGN.md §3 names the files).
inline int env_cfg(const char* name, int dflt) {
  const char* e = rvcx_knob(name);
  return e ? std::atoi(e) : dflt;
}
// contraction arithmetic: 1 = native fp32 MFMA (conv_gemm_kernel), 2 = fp32 through the 3-way bf16 split everywhere
// (conv_emu.hip), 3 (the default) = as 2 except the weight-streamed kernel and the fused ResBlock pairs (the generator),
// which take the two-plane fp16 split (the WSPLIT_H16 / RB_WF16 images: three MFMA products per step instead of six,
// measured as accurate as native fp32, bench_conv / tests/test_gpu_conv_math.py); ConvArgs::math overrides
// RVCX_CONV_MATH (f32 | split | h16)
}  // namespace
int conv_math(int requested) {
  static const int env = [] {
    const char* e = rvcx_knob("RVCX_CONV_MATH");
    if (e && (std::string(e) == "f32" || std::string(e) == "1")) return 1;
    if (e && (std::string(e) == "split" || std::string(e) == "2")) return 2;
    return 3;
  }();
  return requested > 0 ? requested : env;
}
namespace {

// Tile per shape class in split mode, from build/bench_conv on MI355X (TF/s, split vs the native fp32 kernel):
// long-tap convs 128x32 (C128 k11 155 vs 114, C256 k11 138 vs 106), short taps and GEMMs 64x64 (C128 k3 + residual
// 101 vs 78, HuBERT qkv 52 vs 38), narrow short convs (N <= 32, taps < 5: the 32-channel ResBlock k=3, latency
// bound) stay on the native kernel (53 vs 47): both arithmetics are fp32 accurate, so the choice is per shape. The
// U-Net's 3x3 convs: 64x64 (C2 26.7 -> 25.9 ms vs 128x64)
int pick_emu(const ConvArgs& a, bool two_d) {
  if (two_d) return a.N <= 32 ? TILE_EMU_128x32 : TILE_EMU_64x64;
  if (a.N <= 32) return a.taps >= 5 ? TILE_EMU_128x32 : TILE_F32_128x32;
  if (a.taps >= 5) return TILE_EMU_128x32;
  return TILE_EMU_64x64;
}

int pick_cfg(const ConvArgs& a, bool two_d) {
  if (conv_math(a.math) >= 2) return pick_emu(a, two_d);
  // N <= 32 and the 1-D convs with taps >= 5 (A/B: 32.8 vs 33.6 ms): 128 x 32; everything else 64 x 64
  if (a.N <= 32) return TILE_F32_128x32;
  if (!two_d && a.taps >= 5) return TILE_F32_128x32;
  return TILE_F32_64x64;
}

// the LDS-staged tiles, the same two shapes in both arithmetics (ids from 10 on: the bf16 split, conv_emu.hip); an id
// no family has -- the removed tiles' among them -- is refused
inline bool lds_tile(int tile, int& BM, int& BN) {
  const bool wide = tile == TILE_F32_64x64 || tile == TILE_EMU_64x64;
  if (!wide && tile != TILE_F32_128x32 && tile != TILE_EMU_128x32) return false;
  BM = wide ? 64 : 128;
  BN = wide ? 64 : 32;
  return true;
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
  if (a.N <= 32) return TILE_WSB_256x32;
  // the wide ConvTranspose phase group of the second upsample (18600 rows x 1280 columns, 2 taps) on 128 x 128 tiles:
  // bench_conv r06a h25 254.6 vs h27 232.2 TF (the first one, 1550 rows x 3072, loses there: 189 vs 206)
  if (a.taps <= 3 && a.N >= 1024 && plan_rows(a) >= 8192 && a.C_in < 512 && c_long == 0) return TILE_WSB_128x128;
  if (a.taps <= 3) return TILE_WSB_128x64_1x4;
  if (c_long > 0) return c_long;
  return (a.C_in < 256 && a.N >= 128) ? TILE_WSB_128x128 : TILE_WSB_128x64;
}
}  // namespace
const char* conv_kind_name(int k) {
  static const char* const names[CK_COUNT] = {"conv_wsb16_kernel", "conv_wsb_kernel", "conv_gs16_kernel",
                                              "conv_gsw16_kernel", "k_rb_pair", "k_conv2d_h16/k_conv2d_small",
                                              "conv_emu_kernel", "conv_gemm_kernel", "conv_tiny_kernel",
                                              "conv_wst16_kernel", "other"};
  return (k >= 0 && k < CK_COUNT) ? names[k] : "other";
}

namespace {

// Split-K for a launch on BM x BN tiles (gs: the gather-streamed kernels' rules): ksplit, and through slab the floats
// of the partial-tile workspace a split needs
int plan_splitk(const ConvArgs& a, bool two_d, int BM, int BN, bool gs, long long& slab) {
  slab = 0;
  if (a.no_splitk) return 1;
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
  if (!combine_epi && (tiles >= min_tiles || iters < min_iters || (flops < 1.0e8 && iters < 16))) return 1;
  int ks = (int)((target + tiles - 1) / tiles);
  // the gather-streamed kernels keep >= 8 (chunk, tap) steps per slice: below that a slice is all prologue and
  // epilogue and the extra slab + combine launch cost more than the parallelism gains (bench_gs r03s, cold: HuBERT
  // 768 -> 768 ks 1 22.1 us vs ks 4 27.6, TextEncoder 1x1 ks 1 11.6 vs ks 3 14.4, U-Net 196 px ks 8 19.8 vs ks 16
  // 21.8, 3136 px ks 2 20.2 vs ks 6 27.3; the 3072 -> 768 linear keeps ks 4: 48.6 vs 62.8 unsplit)
  constexpr int gs_min_steps = 8;  // same-box C2: 2 17.73, 8 17.72, 16 17.86, 24 17.97 ms
  ks = std::min(ks, gs ? iters / gs_min_steps : iters / 2);
  ks = std::min(ks, 32);
  // the windowed 2-D gather-streamed kernel splits by whole 32-channel chunks (bench_gs: U-Net 784 px ks 8 and 3136 px
  // ks 4 beat the 10 and 6 the step count would give)
  if (gs && two_d && conv_gsw_eligible(a)) ks = std::min(ks, (a.C_in + CK - 1) / CK);
  if (combine_epi && iters >= 2) ks = std::max(ks, 2);
  if (ks < 2) return 1;
  const long long rows = two_d ? (long long)a.T_out * a.W_out : a.T_out;
  slab = std::max((long long)ks * rows * a.N * a.batch * a.batch_inner, tiles_real * ks * BM * BN);
  return ks;
}

// a static weight on the weight-streamed kernel
bool wsb_wants(const ConvArgs& a) {
  if (!conv_wsb_eligible(a)) return false;
  // where it measured faster (bench_conv, profiles/r02i_bench_conv.txt: 128 x 64 tiles of 2 x 2 waves of 64 x 32
  // with the register epilogue; C2 A/B): N >= 64 with >= 2 taps (ResBlock convs at 64-256 channels incl. k = 3, the
  // polyphase ConvTranspose phases; the 64-channel stage on 128x64 tiles beat the fused pair), on a grid that fills
  // the chip
  constexpr int min_taps = 2, min_tiles = 512, min_n = 64;
  if (a.N < min_n || a.taps < min_taps) return false;
  const long long tiles = (long long)((plan_rows(a) + 127) / 128) * ((a.N + 63) / 64) * a.batch;
  return tiles >= min_tiles;
}

constexpr ConvPlan refused{CK_OTHER, TILE_NONE, 1, 0, -1, false, false};
constexpr ConvPlan tiny_plan{CK_TINY, TILE_NONE, 1, 0, -1, false, false};

// the plan of a launch on the weight-streamed tile `tile` (pick_wsb's unless forced); wst: the weight-stationary
// kernel may take it
ConvPlan plan_wsb(const ConvArgs& a, int tile, bool wst) {
  const int math = conv_math(a.math);
  int BM, BN;
  if (!conv_wsb_tile(tile, BM, BN)) return refused;
  ConvPlan p{CK_WSB16, tile, 1, 0, (a.lowp || math == 3) ? WSPLIT_H16 : WSPLIT_BF16, true, false};
  p.ksplit = plan_splitk(a, false, BM, BN, false, p.slab_floats);
  // the short 64 / 128-channel convs on the weight-stationary kernel (conv_wst.hip), which reads the fp16 image
  if (wst && p.ksplit == 1 && p.wsplit_fmt == WSPLIT_H16 && conv_wst_fits(a, false)) {
    p.kind = CK_WST;
    p.tile = TILE_NONE;
  }
  return p;
}

ConvPlan plan_gs(const ConvArgs& a, bool two_d) {
  ConvPlan p{(two_d && conv_gsw_eligible(a)) ? CK_GSW : CK_GS, TILE_GS_64x64, 1, 0,
             conv_math(a.math) == 3 ? WSPLIT_H16 : WSPLIT_BF16, true, false};
  p.ksplit = plan_splitk(a, two_d, 64, 64, true, p.slab_floats);
  return p;
}

// the LDS-staged families on tile `tile`; split_as_gs: the split is the gather-streamed tile's (below)
ConvPlan plan_lds(const ConvArgs& a, bool two_d, int tile, int pipe, bool split_as_gs) {
  int BM, BN;
  if (!lds_tile(tile, BM, BN) || a.nz_har) return refused;  // no kernel with a 16x16 tile store took the noise conv
  // the arithmetic: fp32 through bf16 planes (conv_emu.hip) or native fp32 (conv_gemm.hip)
  ConvPlan p{tile >= 10 ? CK_EMU : CK_GEMM, tile, 1, 0, -1, false, false};
  // plain GEMMs (1-D, one tap, stride 1) take the double-buffered pipeline unless pipe < 0; pipe > 0 forces it
  // (benchmarks)
  p.pipe = !two_d && a.taps == 1 && a.stride == 1 && pipe >= 0;
  if (split_as_gs) BM = BN = 64;
  p.ksplit = plan_splitk(a, two_d, BM, BN, split_as_gs, p.slab_floats);
  return p;
}

// one LDS-staged launch: the planned tile; where its halo does not fit in LDS (long strided taps), the other tile of
// that arithmetic (policy launches only)
hipError_t run_lds(const ConvPlan& p, const ConvArgs& a, bool two_d, bool fallback, hipStream_t s) {
  const bool emu = p.kind == CK_EMU;
  auto run = [&](int c, bool pipe) {
    return emu ? conv_emu_launch(a, c, two_d, pipe, p.ksplit, s) : conv_gemm_launch(a, c, two_d, pipe, p.ksplit, s);
  };
  hipError_t e = run(p.tile, p.pipe);
  if (e == hipErrorInvalidValue && p.pipe) e = run(p.tile, false);  // a forced pipeline on a conv that is no plain GEMM
  if (e == hipErrorInvalidValue && fallback) {
    for (int alt : {emu ? TILE_EMU_64x64 : TILE_F32_64x64, emu ? TILE_EMU_128x32 : TILE_F32_128x32}) {
      if (alt == p.tile) continue;
      e = run(alt, false);
      if (e != hipErrorInvalidValue) break;
    }
  }
  return e;
}

}  // namespace

ConvPlan conv_plan(const ConvArgs& a, bool two_d, bool static_weight, const ConvForce& force) {
  if (a.N <= 0 || a.T_out <= 0 || a.batch <= 0 || a.C_in <= 0 || a.taps <= 0) return refused;
  const int math = conv_math(a.math);
  // the fused noise conv lives in the 16x16 tile stores' unsplit epilogue only (the caller routes it to such a kernel)
  const bool nz = a.nz_har != nullptr;
  if (nz && (two_d || a.nz_C <= 0 || a.nz_stride <= 0 || a.nz_kk != 1 || a.N != a.nz_u * a.nz_C ||
             a.out_map != OUT_ROWS))
    return refused;
  const bool streamed = static_weight && math >= 2;  // only a constant weight has a pre-split image
  ConvPlan p = refused;
  if (force.kind >= 0) {
    // a forced family (numerics tests, benchmarks): it admits the form or the launch is refused
    switch (force.kind) {
      case CK_WSB16:
        if (streamed && conv_wsb_eligible(a, two_d)) p = plan_wsb(a, force.tile >= 0 ? force.tile : pick_wsb(a), false);
        break;
      case CK_WST:
        if (streamed && math == 3 && !a.lowp && conv_wst_fits(a, two_d))
          p = ConvPlan{CK_WST, TILE_NONE, 1, 0, WSPLIT_H16, true, false};
        break;
      case CK_GS:
      case CK_GSW:
        if (streamed && (force.tile < 0 || force.tile == TILE_GS_64x64) && conv_gs_eligible(a, two_d))
          p = plan_gs(a, two_d);
        break;
      case CK_GEMM:
      case CK_EMU:
        if ((force.tile >= 10) == (force.kind == CK_EMU)) p = plan_lds(a, two_d, force.tile, force.pipe, false);
        break;
      default: break;
    }
  } else if (tiny_fits(a)) {
    if (!nz) p = tiny_plan;
  } else if (two_d && conv2d_small_fits(a)) {
    // 3x3 convs with 16/32 channels: 16x16x4 MFMA fragments (conv2d_small.hip); the fp16-split form reads a pre-split
    // image
    p = ConvPlan{CK_SMALL2D, TILE_NONE, 1, 0, math == 3 ? WSPLIT_S2D : -1, math == 3 && static_weight, false};
  } else {
    // a static weight: the weight-streamed kernel (the big 1-D grids, wsb_wants) or the gather-streamed one (the rest
    // with 32-channel chunks and >= 64 outputs)
    // the weight-streamed kernel on small grids (split-K) and on the U-Net's 3x3 convs measured slower than the
    // gather-streamed one (HuBERT / TextEncoder GEMMs +0.7 ms, U-Net +0.8 ms: with few M tiles every wave re-streams its
    // B fragments from L2)
    const bool wsb = streamed && !two_d && wsb_wants(a);
    // everything else with a static weight, 32-channel chunks and >= 64 outputs: the short contractions
    const bool gs = streamed && !wsb && a.N >= 64 && conv_gs_form(a, two_d);
    if (wsb) {
      p = plan_wsb(a, pick_wsb(a), true);
    } else if (gs && !a.lowp) {
      p = plan_gs(a, two_d);
    } else {
      // (a reduced-precision launch of a gather-streamed shape -- those kernels have no such mode -- runs here, split
      // as the gather-streamed tile would be: a short hop's ConvTranspose phases)
      p = plan_lds(a, two_d, pick_cfg(a, two_d), force.pipe, gs);
      if (p.kind != CK_OTHER && p.ksplit == 1 && rows1x1_fits(a, two_d)) p = tiny_plan;
    }
  }
  // the noise conv needs an unsplit launch; the gate and the LayerNorm are applied by the combine
  if ((nz && p.ksplit > 1) || ((a.gate_h > 0 || a.ln_g) && p.ksplit < 2)) return refused;
  return p;
}

hipError_t conv_run(const ConvPlan& p, const ConvArgs& a_in, bool two_d, hipStream_t s, bool forced) {
  if (a_in.N <= 0 || a_in.T_out <= 0 || a_in.batch <= 0) return hipSuccess;
  if (p.kind == CK_OTHER || p.ksplit < 1 || (p.ksplit > 1 && !a_in.ws) ||
      (p.wsplit_fmt >= 0 && p.kind != CK_SMALL2D && !a_in.wsplit))
    return hipErrorInvalidValue;
  // images of different heights (ConvArgs::h_in): a 2-D launch of a family whose gather tests the bound, or an error
  if (a_in.h_in && (!two_d || p.kind == CK_WST || p.kind == CK_WSB16)) return hipErrorInvalidValue;
  // the fields the kernels read from their kernarg copy of the record
  ConvArgs a = a_in;
  a.ksplit = p.ksplit;
  a.ws_rows = two_d ? (long long)a.T_out * a.W_out : a.T_out;
  a.wsplit_fmt = p.wsplit_fmt >= 0 ? p.wsplit_fmt : 0;
  if (p.wsplit_fmt < 0) a.wsplit = nullptr;
  else if (p.kind != CK_SMALL2D) a.wsplit_npad = conv_wsplit_npad(a.N);
  hipError_t e;
  switch (p.kind) {
    case CK_TINY: return tiny_fits(a) ? launch_tiny(a, two_d, s) : launch_rows1x1(a, two_d, s);
    case CK_SMALL2D: return conv2d_small(a, s);
    case CK_WST: return conv_wst_launch(a, s);
    case CK_GS:
    case CK_GSW: e = conv_gs_launch(a, p.tile, s, two_d, p.ksplit); break;
    case CK_WSB16: e = conv_wsb_launch(a, p.tile, s, two_d, p.ksplit); break;
    case CK_EMU:
    case CK_GEMM: e = run_lds(p, a, two_d, !forced, s); break;
    default: return hipErrorInvalidValue;
  }
  if (e == hipSuccess && p.ksplit > 1) e = launch_splitk_reduce(a, p.ksplit, two_d, s);
  return e;
}

}  // namespace rvcx
