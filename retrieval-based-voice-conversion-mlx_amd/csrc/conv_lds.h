// What the two LDS-staged implicit-GEMM families (conv_gemm.hip: native fp32 MFMA; conv_emu.hip: fp32 through three
// bf16 planes) share, each rule written once: the host-side tile geometry and launch, the block's decode into (tile,
// batch entry, split-K slice), the activation gather (LDS row -> source row, the 4-channel load, pre-activation and
// row mask) and the weight tile's global -> register load. Each kernel keeps its own LDS layout and store, its MFMA
// loop and its main loop. Included by those two files only.
#pragma once
#include <algorithm>

#include "conv_common.h"

namespace rvcx {

constexpr int LDS_CK = 32;          // contraction channels per LDS chunk
constexpr int LDS_C4 = LDS_CK / 4;  // float4 groups per chunk row

// Tile geometry of one launch (the kernels take it by value). 1-D: a block owns BM output rows and stages their tap
// halo, nrows_a input rows. 2-D: a block owns an rh x rw pixel window (rh rw <= BM; tiles_w windows per image row)
// and stages the (rh + KH - 1) x (rw + KW - 1) window around it. vec_a / vec_b: every row of the operand starts
// 16-byte aligned, so 4 channels move as one vector. ntn: N tiles per M tile (conv_block_coords).
struct LdsGeom {
  int nrows_a, rw = 0, rh = 0, tiles_w = 1, mtiles, vec_a, vec_b, ksplit, ntn;

  LdsGeom(const ConvArgs& a, int BM, int BN, bool two_d, int ksplit_) : ksplit(ksplit_) {
    if (!two_d) {
      nrows_a = (BM - 1) * a.stride + (a.taps - 1) * a.dil + 1;
      mtiles = (a.T_out + BM - 1) / BM;
    } else {
      rw = a.W_out < BM ? a.W_out : BM;
      rh = BM / rw;
      tiles_w = (a.W_out + rw - 1) / rw;
      mtiles = ((a.T_out + rh - 1) / rh) * tiles_w;
      nrows_a = (rh + a.KH - 1) * (rw + a.KW - 1);
    }
    vec_a = ((a.ldx & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.x) & 15) == 0) && ((a.x_bs & 3) == 0) &&
            ((a.x_bs2 & 3) == 0);
    vec_b = ((a.ldw & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.w) & 15) == 0) && ((a.w_bs & 3) == 0) &&
            ((a.w_bs2 & 3) == 0) && ((a.w_ts & 3) == 0);
    ntn = (a.N + BN - 1) / BN;
  }

  // Launch `kern` (one instantiation; lds_set is that instantiation's raised dynamic-LDS limit, kept by the caller in
  // a static so the attribute is set once, not per launch) with lds_bytes of tiles plus ConvArgs::lds_pad, the
  // occupancy throttle, clamped to the 160 KB a workgroup can hold. hipErrorInvalidValue: the tiles do not fit.
  template <class Kern>
  hipError_t launch(Kern kern, size_t& lds_set, const ConvArgs& a, size_t lds_bytes, hipStream_t s) const {
    constexpr size_t lds_max = 160 * 1024;
    if (lds_bytes > lds_max || a.batch_inner < 1) return hipErrorInvalidValue;
    lds_bytes = std::min(lds_bytes + (size_t)std::max(0, a.lds_pad), lds_max);
    if (lds_bytes > lds_set) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
      if (e != hipSuccess) return e;
      lds_set = lds_bytes;
    }
    const dim3 grid(mtiles * ntn, 1, a.batch * a.batch_inner * ksplit);
    hipLaunchKernelGGL(kern, grid, dim3(CONV_THREADS), lds_bytes, s, a, *this);
    return hipGetLastError();
  }
};
constexpr size_t LDS_SET0 = 64 * 1024;  // the dynamic LDS a kernel may ask for before its limit is raised

// What a block works on: split-K slice zsplit of batch entry zb = (outer b, inner bi), output channels n0.., output
// rows m0.. (1-D) or the pixel window at (h0, w0) (2-D); the entry's operands; the valid input rows Hi (2-D: the
// image's own, ConvArgs::h_in); the staged window's width aw (2-D); the input row of LDS row 0 (1-D).
struct LdsBlock {
  int zsplit, zb, b, bi, n0, m0, h0, w0, Hi, aw, row0;
  const float *X, *W, *PM;  // PM: the input-row mask (1-D only, as ConvArgs says), else null
};

template <int BM, int BN, bool TWO_D>
__device__ __forceinline__ LdsBlock lds_block(const ConvArgs& a, const LdsGeom& g) {
  int bx, by, bz;
  conv_block_coords(g.ntn, bx, by, bz);
  LdsBlock k;
  k.zsplit = bz % g.ksplit;
  k.zb = bz / g.ksplit;
  k.b = k.zb / a.batch_inner;
  k.bi = k.zb % a.batch_inner;
  k.n0 = by * BN;
  k.m0 = TWO_D ? 0 : bx * BM;
  k.h0 = TWO_D ? (bx / g.tiles_w) * g.rh : 0;
  k.w0 = TWO_D ? (bx % g.tiles_w) * g.rw : 0;
  k.X = a.x + (long long)k.b * a.x_bs + (long long)k.bi * a.x_bs2;
  k.W = a.w + (long long)k.b * a.w_bs + (long long)k.bi * a.w_bs2;
  k.PM = (!TWO_D && a.pre_mask) ? a.pre_mask + (long long)k.b * a.pre_mask_bs : nullptr;
  k.Hi = TWO_D ? conv_rows_in(a, k.b) : a.T_in;
  k.aw = TWO_D ? g.rw + a.KW - 1 : 0;
  k.row0 = TWO_D ? 0 : k.m0 * a.stride - a.pad;
  return k;
}

// the block's split-K slice [it0, it1) of `total` main-loop iterations
__device__ __forceinline__ void lds_slice(const LdsGeom& g, const LdsBlock& k, int total, int& it0, int& it1) {
  const int per = (total + g.ksplit - 1) / g.ksplit;
  it0 = k.zsplit * per;
  it1 = min(total, it0 + per);
}

// the LDS row that holds tap 0 of the tile's output row ml (2-D: pixel ml of the rh x rw window, row 0 past it)
template <bool TWO_D>
__device__ __forceinline__ int lds_out_row(const ConvArgs& a, const LdsGeom& g, const LdsBlock& k, int ml) {
  if constexpr (!TWO_D) return ml * a.stride;
  else return (ml < g.rh * g.rw) ? (ml / g.rw) * k.aw + (ml % g.rw) : 0;
}
// and the LDS row offset of a tap from there
template <bool TWO_D>
__device__ __forceinline__ int lds_tap_row(const ConvArgs& a, const LdsBlock& k, int tap) {
  return TWO_D ? (tap / a.KW) * k.aw + (tap % a.KW) : tap * a.dil;
}

// ---- the A gather
// LDS row r of the block's A tile -> its source row (of X, and of the row mask). False: the row lies outside the
// input and reads zero. The only place that tests T_in, the image's own height and W_in.
template <bool TWO_D>
__device__ __forceinline__ bool lds_src_row(const ConvArgs& a, const LdsBlock& k, int r, long long& row) {
  if constexpr (!TWO_D) {
    const int g = k.row0 + r;
    row = g;
    return g >= 0 && g < a.T_in;
  } else {
    const int ah = r / k.aw, awi = r - ah * k.aw;
    const int gh = k.h0 - a.padh + ah, gw = k.w0 - a.padw + awi;
    row = (long long)gh * a.W_in + gw;
    return gh >= 0 && gh < k.Hi && gw >= 0 && gw < a.W_in;
  }
}

// channels c..c+3 of a source row (src points at channel c): one 16-byte load where the caller knows the rows
// aligned (vec_a / vec_b) and the four channels there (vec), else by element, zero from C_in on
__device__ __forceinline__ f32x4 lds_load4(const float* src, int c, int C_in, bool vec) {
  if (vec) return *reinterpret_cast<const f32x4*>(src);
  f32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (c + j < C_in) ? src[j] : 0.f;
  return v;
}

// the row-mask value of a source row (1 without a mask)
__device__ __forceinline__ float lds_row_mask(const LdsBlock& k, long long row) { return k.PM ? k.PM[row] : 1.f; }

// a loaded vector as the MFMA reads it: the pre-activation, then (masked) the row mask on the activated value
__device__ __forceinline__ f32x4 lds_pre4(const ConvArgs& a, f32x4 v, float mk, bool masked) {
  if (a.pre_act != ACT_NONE) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = act_fn(v[j], a.pre_act, a.pre_slope);
  }
  if (masked) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] *= mk;
  }
  return v;
}

// the synchronous staging step: channels c..c+3 of source row `row`, loaded and transformed
__device__ __forceinline__ f32x4 lds_stage4(const ConvArgs& a, const LdsBlock& k, const float* src, int c,
                                            long long row, bool vec) {
  return lds_pre4(a, lds_load4(src, c, a.C_in, vec), lds_row_mask(k, row), k.PM != nullptr);
}

// ---- the B tile (BN rows x 32 channels of one (tap, chunk); weights stored [tap][N][C_in]): global -> registers.
// Thread slot v holds channels 4 (tid % 8).. of tile row 32 v + slab_row, where slab_row (< 32) is the family's
// choice of LDS store order. The row offsets are fixed for the whole kernel and computed once (32-bit: one layer's
// weights are < 2^31 floats).
template <int BN>
struct LdsBLoad {
  static_assert((BN * LDS_C4) % CONV_THREADS == 0, "whole slabs of 32 rows");
  static constexpr int BV = BN * LDS_C4 / CONV_THREADS;  // float4 per thread
  int off[BV];
  bool ok[BV];
  bool fast;  // whole tile in range, 16-byte aligned rows, full chunks: one unconditional vector load per slot
  int c4, vec_b, C_in;

  __device__ __forceinline__ LdsBLoad(const ConvArgs& a, const LdsGeom& g, int n0, int slab_row)
      : c4((threadIdx.x % LDS_C4) << 2), vec_b(g.vec_b), C_in(a.C_in) {
#pragma unroll
    for (int v = 0; v < BV; ++v) {
      const int gn = n0 + 32 * v + slab_row;
      ok[v] = gn < a.N;
      off[v] = gn * a.ldw + c4;
    }
    fast = g.vec_b && (a.C_in % LDS_CK) == 0 && n0 + BN <= a.N;
  }

  // Wt: the tap's weights of the block's batch entry; c0: the chunk's first channel
  __device__ __forceinline__ void load(const float* Wt, int c0, f32x4 (&reg)[BV]) const {
    if (fast) {
#pragma unroll
      for (int v = 0; v < BV; ++v) reg[v] = *reinterpret_cast<const f32x4*>(Wt + c0 + off[v]);
      return;
    }
    const int c = c0 + c4;
#pragma unroll
    for (int v = 0; v < BV; ++v) {
      reg[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok[v] && c < C_in) reg[v] = lds_load4(Wt + c0 + off[v], c, C_in, vec_b && c + 4 <= C_in);
    }
  }
};

}  // namespace rvcx
