// Implicit-GEMM convolution on CDNA4 fp32 MFMA (v_mfma_f32_32x32x2_f32): the native-fp32 LDS-staged family.
//
// It takes what the planner leaves to exact fp32: the narrow short convs (N <= 32, taps < 5) under the default
// arithmetic, and every LDS-staged launch under RVCX_CONV_MATH=f32 -- 1-D convs (time-major [T][C]; grouped: batch
// = group), plain GEMMs (taps = 1), 2-D convs on NHWC images.
//
// Tiling: a 256-thread block (4 waves, one 32x32 fp32 accumulator each) owns BM output rows x BN output channels:
// 128 x 32 (4 x 1 waves) or 64 x 64 (2 x 2), the two tiles the planner names. The A tile is staged once per
// 32-channel chunk with its full tap halo ((BM-1)*stride + (taps-1)*dil + 1 rows, or the (RH+KH-1) x (RW+KW-1) pixel
// window in 2-D), the pre-activation applied on the way into LDS; each tap then re-reads shifted rows of that tile
// (no im2col in HBM). B (weights packed [tap][N][C]) is staged per tap. One ds_read_b128 per operand feeds 4 MFMAs
// (the k-pair of MFMA j is channels {8kk+j, 8kk+4+j}). fp32 in / fp32 accumulate MFMA is a bit-exact fp32 fma chain
// at the FP32 vector peak rate. The block decode, the gather and the weight load are conv_lds.h's.
#include "conv_lds.h"

namespace rvcx {

template <int BM, int BN, int WM, int WN, bool TWO_D, bool PIPE>
__global__ __launch_bounds__(CONV_THREADS, 2) void conv_gemm_kernel(const ConvArgs a, const LdsGeom g) {
  constexpr int NT = CONV_THREADS, CK = LDS_CK, C4 = LDS_C4;
  constexpr int CKP = CK + 4;  // padded LDS row: rows i..i+15 land on distinct 16-B bank slots
  static_assert(WM * WN == 4 && BM == WM * 32 && BN == WN * 32, "4 waves, one 32x32 accumulator each");
  static_assert(!(PIPE && TWO_D), "the GEMM pipeline is 1-D");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;
  float* Bs0 = smem + g.nrows_a * CKP;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, hk = lane >> 5;
  const LdsBlock k = lds_block<BM, BN, TWO_D>(a, g);
  const int base = lds_out_row<TWO_D>(a, g, k, wm * 32 + li);

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  const LdsBLoad<BN> bload(a, g, k.n0, tid / C4);
  constexpr int BV = LdsBLoad<BN>::BV;
  auto load_b = [&](int tap, int c0, f32x4 (&reg)[BV]) { bload.load(k.W + (long long)tap * a.w_ts, c0, reg); };
  auto store_b = [&](float* Bs, const f32x4 (&reg)[BV]) {
#pragma unroll
    for (int v = 0; v < BV; ++v)
      *reinterpret_cast<f32x4*>(&Bs[(32 * v + tid / C4) * CKP + ((tid % C4) << 2)]) = reg[v];
  };
  // A tile: nrows_a x 32 channels of chunk c0 -> LDS, pre-activation applied, zero outside the input
  auto stage_a = [&](int c0) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if constexpr (!TWO_D) {
      // 1-D: a thread keeps one 4-channel column and walks rows NT / C4 apart, so the source and LDS addresses
      // advance by constants (no per-element 64-bit index math)
      constexpr int RSTEP = NT / C4;
      const int c4 = (tid % C4) << 2;
      const int c = c0 + c4;
      const bool cv = g.vec_a && c + 4 <= a.C_in;
      int r = tid / C4;
      const float* src = k.X + (long long)(k.row0 + r) * a.ldx + c;
      const long long src_step = (long long)RSTEP * a.ldx;
      for (; r < g.nrows_a; r += RSTEP, src += src_step) {
        long long row;
        const bool ok = lds_src_row<false>(a, k, r, row) && c < a.C_in;
        *reinterpret_cast<f32x4*>(&As[r * CKP + c4]) = ok ? lds_stage4(a, k, src, c, row, cv) : zero;
      }
    } else {
      for (int idx = tid; idx < g.nrows_a * C4; idx += NT) {
        const int r = idx / C4;
        const int c4 = (idx % C4) << 2;
        const int c = c0 + c4;
        const bool cv = g.vec_a && c + 4 <= a.C_in;
        long long row;
        const bool ok = lds_src_row<true>(a, k, r, row) && c < a.C_in;
        *reinterpret_cast<f32x4*>(&As[r * CKP + c4]) =
            ok ? lds_stage4(a, k, k.X + row * a.ldx + c, c, row, cv) : zero;
      }
    }
  };
  auto compute = [&](const float* Bs, int tap) {
    const int toff = lds_tap_row<TWO_D>(a, k, tap);
#pragma unroll
    for (int kk = 0; kk < CK; kk += 8) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(&As[(base + toff) * CKP + kk + hk * 4]);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(&Bs[(wn * 32 + li) * CKP + kk + hk * 4]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
    }
  };

  const int nchunks = (a.C_in + CK - 1) / CK;
  f32x4 breg[BV];
  int it0, it1;
  if constexpr (!PIPE) {
    lds_slice(g, k, nchunks * a.taps, it0, it1);
    int it = it0;
    while (it < it1) {
      const int ch = it / a.taps;
      __syncthreads();
      stage_a(ch * CK);
      for (int tap = it - ch * a.taps; tap < a.taps && it < it1; ++tap, ++it) {
        if (it > it0 && tap != it0 - ch * a.taps) __syncthreads();
        load_b(tap, ch * CK, breg);
        store_b(Bs0, breg);
        __syncthreads();
        compute(Bs0, tap);
      }
    }
  } else {
    // PIPE (1-D, taps == 1, stride 1: a plain GEMM over C_in): A and B both double-buffered in LDS; the next
    // chunk's tiles are fetched into registers while the MFMAs consume the current ones, then written to
    // the other buffers; one barrier per chunk. Small-M GEMMs (HuBERT at 775 rows, TextEncoder/flow at
    // 1550) otherwise expose two dependent global-load latencies per 32-channel chunk.
    constexpr int AV = BM * C4 / NT;
    float* const A0 = smem;
    float* const A1 = smem + BM * CKP;
    float* const B0 = smem + 2 * BM * CKP;
    float* const B1 = B0 + BN * CKP;
    f32x4 areg[AV];
    float amk[AV];  // 0 outside the input, else the row mask
    auto load_a = [&](int c0) {
      const int c = c0 + ((tid % C4) << 2);
      const bool cv = g.vec_a && c + 4 <= a.C_in;
#pragma unroll
      for (int v = 0; v < AV; ++v) {
        long long row;
        areg[v] = f32x4{0.f, 0.f, 0.f, 0.f};
        amk[v] = 0.f;
        if (lds_src_row<false>(a, k, v * (NT / C4) + tid / C4, row) && c < a.C_in) {
          amk[v] = lds_row_mask(k, row);
          areg[v] = lds_load4(k.X + row * a.ldx + c, c, a.C_in, cv);
        }
      }
    };
    auto store_a = [&](float* dst) {
#pragma unroll
      for (int v = 0; v < AV; ++v) {
        const f32x4 val = amk[v] != 0.f ? lds_pre4(a, areg[v], amk[v], k.PM != nullptr) : f32x4{0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(&dst[(v * (NT / C4) + tid / C4) * CKP + ((tid % C4) << 2)]) = val;
      }
    };
    lds_slice(g, k, nchunks, it0, it1);
    if (it0 < it1) {
      load_a(it0 * CK);
      load_b(0, it0 * CK, breg);
      store_a(A0);
      store_b(B0, breg);
      __syncthreads();
      for (int it = it0; it < it1; ++it) {
        const bool odd = (it - it0) & 1;
        const bool more = it + 1 < it1;
        if (more) {
          load_a((it + 1) * CK);
          load_b(0, (it + 1) * CK, breg);
        }
        As = odd ? A1 : A0;
        compute(odd ? B1 : B0, 0);
        if (more) {
          store_a(odd ? A0 : A1);
          store_b(odd ? B0 : B1, breg);
        }
        __syncthreads();
      }
    }
  }

  conv_store_tile<WN, TWO_D>(a, TilePos{k.m0, k.h0, k.w0, g.rw, g.rh, k.n0, k.b, k.bi, k.zb, k.zsplit, g.ksplit}, acc);
}

namespace {

template <int BM, int BN, int WM, int WN, bool TWO_D, bool PIPE>
hipError_t launch_cfg(const ConvArgs& a, int ksplit, hipStream_t s) {
  if (PIPE && (a.taps != 1 || a.stride != 1)) return hipErrorInvalidValue;
  const LdsGeom g(a, BM, BN, TWO_D, ksplit);
  static size_t lds_set = LDS_SET0;
  // A [nrows_a] | B [BN] rows of 36 floats; the GEMM pipeline holds two of each (nrows_a = BM there)
  return g.launch(conv_gemm_kernel<BM, BN, WM, WN, TWO_D, PIPE>, lds_set, a,
                  (size_t)(PIPE ? 2 : 1) * (g.nrows_a + BN) * (LDS_CK + 4) * sizeof(float), s);
}

template <int BM, int BN, int WM, int WN>
hipError_t launch_tile(const ConvArgs& a, bool two_d, bool pipe, int ksplit, hipStream_t s) {
  if (two_d) return pipe ? hipErrorInvalidValue : launch_cfg<BM, BN, WM, WN, true, false>(a, ksplit, s);
  return pipe ? launch_cfg<BM, BN, WM, WN, false, true>(a, ksplit, s)
              : launch_cfg<BM, BN, WM, WN, false, false>(a, ksplit, s);
}

}  // namespace

// a split launch (ksplit > 1) leaves the combine to the caller, as conv_emu_launch does; hipErrorInvalidValue: the
// tile's LDS does not fit, the tile is not this family's, or it has no such form
hipError_t conv_gemm_launch(const ConvArgs& a, int cfg, bool two_d, bool pipe, int ksplit, hipStream_t s) {
  switch (cfg) {
    case TILE_F32_128x32: return launch_tile<128, 32, 4, 1>(a, two_d, pipe, ksplit, s);
    case TILE_F32_64x64: return launch_tile<64, 64, 2, 2>(a, two_d, pipe, ksplit, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace rvcx
