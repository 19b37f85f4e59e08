// Shared pieces of the implicit-GEMM conv kernels (conv_gemm.hip: exact fp32 MFMA; conv_emu.hip: fp32 through
// three bf16 planes; the streamed kernels): activations, the fused epilogue, the accumulator -> HBM store of one block
// tile, and what the conv translation units declare to each other.
#pragma once
#include "conv_kernels.h"

namespace rvcx {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CONV_THREADS = 256;  // 4 waves per block in every conv kernel

static __device__ __noinline__ float act_fn_slow(float v, int act, float slope) {
  switch (act) {
    case ACT_GELU: return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
    case ACT_TANH: return tanhf(v);
    case ACT_SIGMOID: return 1.f / (1.f + expf(-v));
    case ACT_LOGCLAMP: return logf(fmaxf(v, slope));
    default: return v;
  }
}

// cheap activations inline, transcendental ones out of line (keeps the unrolled epilogue small
// enough that the accumulators stay in registers)
static __device__ __forceinline__ float act_fn(float v, int act, float slope) {
  if (act == ACT_NONE) return v;
  if (act == ACT_LRELU) return v > 0.f ? v : v * slope;
  if (act == ACT_RELU) return v > 0.f ? v : 0.f;
  return act_fn_slow(v, act, slope);
}

// Pre-activation chosen at compile time (kernel MODE bits 0-1: 0 none, 1 leaky ReLU, 2 any other via act_fn): a
// runtime act switch per element put ~30-120 scalar branches into every A staging pass of the streamed kernels
enum { PA_NONE = 0, PA_LRELU = 1, PA_ANY = 2 };
template <int PA>
static __device__ __forceinline__ float pre_fn(float v, int act, float slope) {
  if constexpr (PA == PA_NONE) return v;
  else if constexpr (PA == PA_LRELU) return v > 0.f ? v : v * slope;
  else return act_fn(v, act, slope);
}
static inline int pre_mode(int act) { return act == ACT_NONE ? PA_NONE : (act == ACT_LRELU ? PA_LRELU : PA_ANY); }

// The valid input rows of outer batch entry b: its own height in a batch of images of different heights
// (ConvArgs::h_in), else T_in. b has to be uniform over the wave (the block's batch index, or a readfirstlane): the
// bound is then one scalar load, and every gather tests its row against it where it tested T_in.
// The heights are written by the host before the launch and by no kernel: read through the constant address space, the
// load is scalar (s_load_dword) also where it sits in a loop beside stores the compiler cannot tell apart from it.
static __device__ __forceinline__ int conv_rows_in(const ConvArgs& a, int b) {
  typedef const int __attribute__((address_space(4))) * const_ip;
  return a.h_in ? ((const_ip)a.h_in)[b] : a.T_in;
}

// The fused epilogue, defined once for every kernel that takes its switches at run time:
//   bias -> pre-residual -> alpha -> activation -> post-residual / reverse-subtract -> accumulate (/ div)  [epi_math]
//   -> noise conv [epi_noise] -> mask [epi_mask] -> store.
// A caller decides which accumulator element is which output (row, column), gathers the residual / accumulate / mask
// operands (always before its first store: the stores may alias them, an in-place residual reads the very element it
// writes, so the compiler cannot hoist the loads itself) and stores. conv_wst16_kernel and the fused ResBlock pair
// keep epilogues of their own with compile-time switches, in this order of operations.

// the batch entry's (outer b, inner bi) epilogue operands and output
struct EpiPtrs {
  const float *bias, *R, *MK;
  float* Y;
};
__device__ __forceinline__ EpiPtrs epi_ptrs(const ConvArgs& a, int b, int bi) {
  return {a.bias ? a.bias + (long long)b * a.bias_bs + (long long)bi * a.bias_bs2 : nullptr,
          a.res ? a.res + (long long)b * a.res_bs + (long long)bi * a.res_bs2 : nullptr,
          a.mask ? a.mask + (long long)b * a.mask_bs : nullptr, a.y + (long long)b * a.y_bs + (long long)bi * a.y_bs2};
}

// element r of a group's operand: one float for the whole group, or one per element (a vector, an array, a pointer)
__device__ __forceinline__ float epi_at(float x, int) { return x; }
template <class T>
__device__ __forceinline__ float epi_at(const T& x, int r) {
  return x[r];
}

// bias .. accumulate on a group of W values v (bn: the bias, rv: the residual, dv: the destination's old value; each
// a float or indexable by element). The switches are uniform and tested once per group, each around its group-wide
// operation: tested per element they cost ~25 scalar branches per output, as much as a short tile's MMA loop. Cheap
// activations inline, the transcendental ones out of line (act_fn).
template <int W, class V, class BN, class RV, class DV>
__device__ __forceinline__ void epi_math(const ConvArgs& a, V& v, const BN& bn, const RV& rv, const DV& dv) {
  const int act = a.act;
  if (a.bias) {
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] += epi_at(bn, r);
  }
  if (a.res_mode == RES_ADD_PRE) {
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] = v[r] + epi_at(rv, r);
  }
  if (a.alpha != 1.f) {
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] *= a.alpha;
  }
  if (act == ACT_LRELU) {
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] = v[r] > 0.f ? v[r] : v[r] * a.slope;
  } else if (act == ACT_RELU) {
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] = v[r] > 0.f ? v[r] : 0.f;
  } else if (act != ACT_NONE) {
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] = act_fn_slow(v[r], act, a.slope);
  }
  if (a.res_mode == RES_ADD_POST) {
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] = v[r] + epi_at(rv, r);
  } else if (a.res_mode == RES_RSUB_POST) {
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] = epi_at(rv, r) - v[r];
  }
  if (a.acc_mode == ACC_ADD) {
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] = epi_at(dv, r) + v[r];
  } else if (a.acc_mode == ACC_ADD_DIV) {
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] = (epi_at(dv, r) + v[r]) / a.acc_div;
  }
}

// the NSF noise conv's term (ConvArgs::nz_*, one tap: the dispatcher admits nz_kk = 1 only) of output row m, column n
// of batch entry b: k_noise_add's arithmetic, y + (w x + b) with the product an fma onto 0
__device__ __forceinline__ float epi_noise(const ConvArgs& a, int b, long long m, int n) {
  const int p = n / a.nz_C, c = n - p * a.nz_C;
  const float x = a.nz_har[(long long)b * a.nz_bs + (m * a.nz_u + p) * a.nz_stride];
  return fmaf(a.nz_w[(long long)c * a.nz_stride], x, 0.f) + a.nz_b[c];
}

// the output-row mask, after the noise conv
template <int W, class V, class MV>
__device__ __forceinline__ void epi_mask(const float* MK, V& v, const MV& mv) {
  if (MK) {
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] *= epi_at(mv, r);
  }
}

// one output element (m, n), 2-D pixel (oh, ow): the epilogue and the store (the OUT_UPSAMPLE2D scatter included)
static __device__ __forceinline__ void epilogue_store(const ConvArgs& a, float v, float bn, long long m, int n, int oh,
                                                      int ow, const EpiPtrs& e) {
  float* dst;
  if (a.out_map == OUT_UPSAMPLE2D) {
    const int cv = a.out_cv;
    const int ph = n / (2 * cv), pw = (n / cv) & 1, co = n % cv;
    dst = e.Y + ((long long)(2 * oh + ph) * (2 * a.W_out) + (2 * ow + pw)) * a.ldy + co;
  } else {
    dst = e.Y + m * a.ldy + n;
  }
  // one element has nothing to gather: the operands go in as pointers, read where a switch asks for them
  float v1[1] = {v};
  epi_math<1>(a, v1, bn, e.R + (m * a.ldr + n), dst);
  epi_mask<1>(e.MK, v1, e.MK + m);
  *dst = v1[0];
}

// The 16x16 accumulator tiles of a wave (v_mfma_f32_16x16x32 C layout: lane l holds column l % 16, rows 4 (l / 16) + r)
// -> HBM or the split-K slab, with the shared epilogue on the 4 rows of a column.
// UP2D: the instantiation may see the ConvTranspose2d phase layout (OUT_UPSAMPLE2D: the 2-D gather-streamed kernel
// only; compiled out elsewhere)
template <int TM16, int TN16, int WM, int WN, bool UP2D = false>
__device__ __forceinline__ void store_tile16(const ConvArgs& a, int m0, int n0, int b, int zsplit, int ksplit,
                                             long long Mtot, f32x4 (&acc)[TM16][TN16]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lc = lane & 15, lg = lane >> 4;
  if (ksplit > 1) {
#pragma unroll
    for (int tn = 0; tn < TN16; ++tn) {
      const int n = n0 + wn * TN16 * 16 + tn * 16 + lc;
#pragma unroll
      for (int tm = 0; tm < TM16; ++tm) {
        const long long mb = (long long)m0 + wm * TM16 * 16 + tm * 16 + 4 * lg;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n < a.N && mb + r < Mtot) a.ws[(((long long)b * ksplit + zsplit) * a.ws_rows + mb + r) * a.N + n] = acc[tm][tn][r];
      }
    }
    return;
  }
  const EpiPtrs e = epi_ptrs(a, b, 0);
  const float* R = e.R;
  const float* MK = e.MK;
  float* Y = e.Y;
  const bool need_r = R && a.res_mode != RES_NONE;
  const bool need_d = a.acc_mode != ACC_STORE;
#pragma unroll
  for (int tn = 0; tn < TN16; ++tn) {
    const int n = n0 + wn * TN16 * 16 + tn * 16 + lc;
    const bool n_ok = n < a.N;
    const float bn = (e.bias && n_ok) ? e.bias[n] : 0.f;
#pragma unroll
    for (int tm = 0; tm < TM16; ++tm) {
      const long long mb = (long long)m0 + wm * TM16 * 16 + tm * 16 + 4 * lg;
      bool ok[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) ok[r] = n_ok && mb + r < Mtot;
      f32x4 v = acc[tm][tn];
      f32x4 rv = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f}, mv = {1.f, 1.f, 1.f, 1.f};
      if (need_r) {
#pragma unroll
        for (int r = 0; r < 4; ++r) rv[r] = ok[r] ? R[(mb + r) * a.ldr + n] : 0.f;
      }
      if (need_d) {
#pragma unroll
        for (int r = 0; r < 4; ++r) dv[r] = ok[r] ? Y[(mb + r) * a.ldy + n] : 0.f;
      }
      if (MK) {
#pragma unroll
        for (int r = 0; r < 4; ++r) mv[r] = ok[r] ? MK[mb + r] : 1.f;
      }
      epi_math<4>(a, v, bn, rv, dv);
      if (a.nz_har && n_ok) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = v[r] + epi_noise(a, b, ok[r] ? mb + r : 0, n);
      }
      epi_mask<4>(MK, v, mv);
      if (UP2D && a.out_map == OUT_UPSAMPLE2D) {
        // the 2x2-phase ConvTranspose2d (epilogue_store's mapping): virtual column n = (ph, pw, co) of input pixel m
        const int cv = a.out_cv;
        const int ph = n / (2 * cv), pw = (n / cv) & 1, co = n - (n / cv) * cv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (!ok[r]) continue;
          const long long m = mb + r;
          const long long oh = m / a.W_out, ow = m - oh * a.W_out;
          Y[((2 * oh + ph) * (2 * a.W_out) + (2 * ow + pw)) * a.ldy + co] = v[r];
        }
        continue;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (ok[r]) Y[(mb + r) * a.ldy + n] = v[r];
    }
  }
}

// store_tile16 for the transposed accumulator layout D = W X^T (conv_wsb.hip): lane (lc, lg) of a 16x16 tile holds
// row lc, columns 4 lg + r, so the residual / accumulate operands and the outputs move as one 16-byte vector per lane
// and tile where the rows are 16-byte aligned (vec: N, the row strides and the bases multiples of 4 floats) -- a
// quarter of store_tile16's memory instructions, whose issue rate, not HBM, bounded the epilogue. 1-D OUT_ROWS only.
template <int TM16, int TN16, int WM, int WN>
__device__ __forceinline__ void store_tile16t(const ConvArgs& a, int m0, int n0, int b, int zsplit, int ksplit,
                                              long long Mtot, f32x4 (&acc)[TM16][TN16]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lc = lane & 15, lg = lane >> 4;
  const bool nvec = (a.N & 3) == 0;
  if (ksplit > 1) {
    float* W = a.ws + ((long long)b * ksplit + zsplit) * a.ws_rows * a.N;
#pragma unroll
    for (int tm = 0; tm < TM16; ++tm) {
      const long long m = (long long)m0 + wm * TM16 * 16 + tm * 16 + lc;
      if (m >= Mtot) continue;
#pragma unroll
      for (int tn = 0; tn < TN16; ++tn) {
        const int n = n0 + wn * TN16 * 16 + tn * 16 + 4 * lg;
        float* dst = W + m * a.N + n;
        if (nvec && n + 3 < a.N) {
          *reinterpret_cast<f32x4*>(dst) = acc[tm][tn];
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n + r < a.N) dst[r] = acc[tm][tn][r];
        }
      }
    }
    return;
  }
  const EpiPtrs e = epi_ptrs(a, b, 0);
  const float* R = e.R;
  const float* MK = e.MK;
  float* Y = e.Y;
  const bool need_r = R && a.res_mode != RES_NONE;
  const bool need_d = a.acc_mode != ACC_STORE;
  const bool vec = nvec && ((reinterpret_cast<uintptr_t>(Y) & 15) == 0) && (a.ldy & 3) == 0 &&
                   (!need_r || (((reinterpret_cast<uintptr_t>(R) & 15) == 0) && (a.ldr & 3) == 0));
#pragma unroll
  for (int tn = 0; tn < TN16; ++tn) {
    const int n = n0 + wn * TN16 * 16 + tn * 16 + 4 * lg;
    f32x4 bn = {0.f, 0.f, 0.f, 0.f};
    if (e.bias) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bn[r] = n + r < a.N ? e.bias[n + r] : 0.f;
    }
#pragma unroll
    for (int tm = 0; tm < TM16; ++tm) {
      const long long m = (long long)m0 + wm * TM16 * 16 + tm * 16 + lc;
      const bool m_ok = m < Mtot;
      const bool full = m_ok && n + 3 < a.N;
      bool ok[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) ok[r] = m_ok && n + r < a.N;
      f32x4 v = acc[tm][tn];
      f32x4 rv = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
      float mv = 1.f;
      if (need_r) {
        const float* src = R + m * a.ldr + n;
        if (vec && full) {
          rv = *reinterpret_cast<const f32x4*>(src);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) rv[r] = ok[r] ? src[r] : 0.f;
        }
      }
      if (need_d) {
        const float* src = Y + m * a.ldy + n;
        if (vec && full) {
          dv = *reinterpret_cast<const f32x4*>(src);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) dv[r] = ok[r] ? src[r] : 0.f;
        }
      }
      if (MK) mv = m_ok ? MK[m] : 1.f;
      epi_math<4>(a, v, bn, rv, dv);
      if (a.nz_har) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ok[r]) v[r] = v[r] + epi_noise(a, b, m, n + r);
      }
      epi_mask<4>(MK, v, mv);
      float* dst = Y + m * a.ldy + n;
      if (vec && full) {
        *reinterpret_cast<f32x4*>(dst) = v;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ok[r]) dst[r] = v[r];
      }
    }
  }
}

// Where a block tile sits: output rows m0.. (1-D) or the rh x rw pixel window at (h0, w0) (2-D), output channels
// n0.., outer/inner batch (b, bi), split-K slice zsplit of ksplit for batch entry zb.
struct TilePos {
  int m0, h0, w0, rw, rh, n0, b, bi, zb, zsplit, ksplit;
};

// The block's accumulators -> HBM, straight from registers. Wave (wm, wn) of the block's WM x WN holds one 32x32 tile
// in the MFMA C layout: lane (li, hk), register r is row (r&3) + 8(r>>2) + 4hk, column li. Split-K slices write their
// partial tile to the slab (splitk_reduce_kernel applies the epilogue); otherwise the fused epilogue runs here.
template <int WN, bool TWO_D>
__device__ __forceinline__ void conv_store_tile(const ConvArgs& a, const TilePos& p, const f32x16& acc) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, hk = lane >> 5;
  const EpiPtrs e = epi_ptrs(a, p.b, p.bi);
  const float *bias = e.bias, *R = e.R, *MK = e.MK;
  float* Y = e.Y;
  auto emit = [&](float v, int ml, int n, bool n_ok, float bn) {
    long long m;
    int oh = 0, ow = 0;
    bool ok;
    if (!TWO_D) {
      m = p.m0 + ml;
      ok = n_ok && (m < a.T_out);
    } else {
      oh = p.h0 + ml / p.rw;
      ow = p.w0 + ml % p.rw;
      ok = n_ok && (ml < p.rh * p.rw) && (oh < a.T_out) && (ow < a.W_out);
      m = (long long)oh * a.W_out + ow;
    }
    if (ok) {
      if (p.ksplit > 1) {
        a.ws[(((long long)p.zb * p.ksplit + p.zsplit) * a.ws_rows + m) * a.N + n] = v;
      } else {
        epilogue_store(a, v, bn, m, n, oh, ow, e);
      }
    }
  };
  const int n = p.n0 + wn * 32 + li;
  const bool n_ok = n < a.N;
  const float bn = (bias && n_ok) ? bias[n] : 0.f;
  if (!TWO_D && p.ksplit == 1 && a.out_map == OUT_ROWS) {
    // 1-D rows, gather first: the residual, accumulate and mask operands of the lane's 16 outputs are all loaded
    // before the first store. The stores may alias them (an in-place residual reads the very element it writes), so
    // the compiler cannot hoist the loads across the stores itself and would expose one load latency per output
    // (16 per lane): the short-contraction convs (ResBlock k=3 at 32/64 channels) were latency-bound on exactly
    // that. Each element is read and written by this lane only, so the reorder is exact.
    const bool need_r = R && a.res_mode != RES_NONE;
    const bool need_d = a.acc_mode != ACC_STORE;
    // element r sits at row mb + (r&3) + 8(r>>2) of column n: per-lane base pointers, constant row offsets
    const int mb = p.m0 + wm * 32 + 4 * hk;
    const bool full = p.m0 + wm * 32 + 32 <= a.T_out;
    const float* Rl = need_r ? R + (long long)mb * a.ldr + n : nullptr;
    float* Yl = Y + (long long)mb * a.ldy + n;
    const float* Ml = MK ? MK + mb : nullptr;
    auto row_ok = [&](int r) { return n_ok && (full || mb + (r & 3) + 8 * (r >> 2) < a.T_out); };
    // two halves of 8 elements: one exposed load latency each, 24 staging registers instead of 48 (the
    // VGPR count sets the workgroups per CU of this latency-bound kernel)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float rv[8], dv[8], mv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int r = 8 * h + i;
        const int ro = (r & 3) + 8 * (r >> 2);
        const bool ok = row_ok(r);
        rv[i] = (ok && need_r) ? Rl[ro * a.ldr] : 0.f;
        dv[i] = (ok && need_d) ? Yl[ro * a.ldy] : 0.f;
        mv[i] = (ok && MK) ? Ml[ro] : 1.f;
      }
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = acc[8 * h + i];
      epi_math<8>(a, v, bn, rv, dv);
      epi_mask<8>(MK, v, mv);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int r = 8 * h + i;
        if (row_ok(r)) Yl[((r & 3) + 8 * (r >> 2)) * a.ldy] = v[i];
      }
    }
    return;
  }
  // every other form (2-D, the split-K slab, the ConvTranspose2d scatter): fully unrolled, 16 values per lane
#pragma unroll
  for (int r = 0; r < 16; ++r) emit(acc[r], wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hk, n, n_ok, bn);
}

// Block -> tile: the grid is 1-D over (M tile, N tile) with N fastest when ntn > 0, and the linear workgroup id
// is remapped so each XCD (workgroups are dealt to the 8 XCDs round-robin) owns one contiguous run of tiles: the
// N tiles of an M tile then share its A halo through one L2 instead of re-reading it from HBM/L3 (bijective
// remap, cdna_hip_programming.md T1). ntn = 0: the plain (x = M, y = N) grid.
__device__ __forceinline__ void conv_block_coords(int ntn, int& bx, int& by, int& bz) {
  bx = blockIdx.x;
  by = blockIdx.y;
  bz = blockIdx.z;
  if (ntn > 0) {
    const int X = gridDim.x, total = X * gridDim.z;
    const int orig = blockIdx.z * X + blockIdx.x;
    const int xcd = orig & 7, q = total >> 3, r = total & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    bz = wg / X;
    const int t = wg - bz * X;
    bx = t / ntn;
    by = t - bx * ntn;
  }
}

// One tile of the LDS-staged kernels: conv_gemm.hip (native fp32 MFMA, TILE_F32_*) and conv_emu.hip (fp32 through a
// 3-way bf16 operand split, TILE_EMU_*). pipe: the double-buffered GEMM form; a split launch (ksplit > 1) writes the
// slab and leaves the combine to the caller. hipErrorInvalidValue: the tile's LDS does not fit, the tile is not that
// family's, or it has no such form
hipError_t conv_gemm_launch(const ConvArgs& a, int cfg, bool two_d, bool pipe, int ksplit, hipStream_t s);
hipError_t conv_emu_launch(const ConvArgs& a, int cfg, bool two_d, bool pipe, int ksplit, hipStream_t s);
// conv_tiny.hip: the one-thread-per-output kernels, the shapes they take and their launches
bool tiny_fits(const ConvArgs& a);
bool rows1x1_fits(const ConvArgs& a, bool two_d);
hipError_t launch_tiny(const ConvArgs& a, bool two_d, hipStream_t s);
hipError_t launch_rows1x1(const ConvArgs& a, bool two_d, hipStream_t s);
// conv_splitk.hip: the combine of a split launch (slab sum + the shared epilogue, the LayerNorm or the gate)
hipError_t launch_splitk_reduce(const ConvArgs& a, int ksplit, bool two_d, hipStream_t s);

}  // namespace rvcx
