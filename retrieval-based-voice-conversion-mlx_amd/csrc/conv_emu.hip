// fp32 implicit-GEMM convolution on CDNA4 bf16 MFMA (v_mfma_f32_32x32x16_bf16) through a 3-way operand split.
//
// gfx950 has no xf32: its fp32-input MFMA (conv_gemm.hip) runs at the FP32 vector rate, 1/16 of bf16. Every
// fp32 operand x is split exactly into three bf16 planes, x = x0 + x1 + x2 (x0 = bf16(x), x1 = bf16(x - x0),
// x2 = bf16(x - x0 - x1); each difference is exact in fp32 and the three planes carry all 24 significand bits),
// and a product is summed as the six plane products with i + j <= 2:
//     x*y ~= x2*y0 + x1*y1 + x0*y2 + x1*y0 + x0*y1 + x0*y0        (smallest first, one fp32 accumulator)
// Each bf16 x bf16 product is exact in fp32; the dropped terms x1*y2 + x2*y1 + x2*y2 are below 2^-25 |x*y|, under
// the fp32 rounding every fma of the native path incurs. So the contraction is fp32 accurate (no reduced
// precision anywhere: tests/test_gpu_conv_math.py measures the error against fp64 next to the native fp32 MFMA
// path) at 6 x 32 cycles per 32x32x16 step instead of 8 x 64 for the f32 form: 2.67x the MFMA throughput.
//
// The split happens once, on the way into LDS (A: the halo tile of one 32-channel chunk, reused by every tap;
// B: the per-tap weight tile), so the MFMA loop reads ready bf16 fragments. LDS row = [hi | mid | lo] x 32
// channels + 16 B pad (208 B = 52 dwords: 16 consecutive rows hit 16 distinct 4-bank groups). B is double
// buffered with a one-tap register prefetch (one barrier per tap); A is staged per chunk for the halo convs (1-D
// from registers loaded one chunk ahead, 2-D synchronously), double buffered with register prefetch for plain GEMMs
// (taps 1, stride 1).
//
// Tiles: 128 x 32 (4 x 1 waves) and 64 x 64 (2 x 2), one 32x32 accumulator per wave; each as a 1-D, a 1-D GEMM-pipeline
// and a 2-D kernel. The block decode, the gather and the weight load are conv_lds.h's, shared with conv_gemm.hip.
#include "conv_lds.h"
#include "split_bf16.h"

namespace rvcx {

namespace {

using namespace splitbf16;
static_assert(EK == LDS_CK, "the chunk of the shared scaffold");

// (launch bound: four blocks per CU, which holds every form to 128 registers. At two the 64 x 64 1-D form takes one
// more, for spilled scalars, and loses a wave per SIMD: profiles/lds_scaffold_resources.txt)
template <int BM, int BN, int WM, int WN, bool TWO_D, bool PIPE>
__global__ __launch_bounds__(CONV_THREADS, 4) void conv_emu_kernel(const ConvArgs a, const LdsGeom g) {
  constexpr int NT = CONV_THREADS;
  static_assert(WM * WN == 4 && BM == WM * 32 && BN == WN * 32, "4 waves, one 32x32 accumulator each");
  static_assert(!(PIPE && TWO_D), "the GEMM pipeline is 1-D");
  extern __shared__ __attribute__((aligned(16))) char smem_e[];
  // non-PIPE: A [nrows_a] | B0 [BN] | B1 [BN] ; PIPE: A0 [BM] | A1 [BM] | B0 | B1   (rows of ERS bytes)
  char* const A0 = smem_e;
  char* const A1 = PIPE ? smem_e + BM * ERS : smem_e;
  char* const B0 = smem_e + (PIPE ? 2 * BM : g.nrows_a) * ERS;
  char* const B1 = B0 + BN * ERS;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, hk = lane >> 5;
  const LdsBlock k = lds_block<BM, BN, TWO_D>(a, g);

  // byte offsets of this lane's fragment rows (tap 0, K16 step 0)
  const int aoff = lds_out_row<TWO_D>(a, g, k, wm * 32 + li) * ERS + hk * 16;
  const int boff = (wn * 32 + li) * ERS + hk * 16;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  // a thread's float4 of a staged tile: channels c4.. of row 32 v + srow (store_row: the bank-conflict-free order)
  const int srow = store_row(tid / EC4), c4 = (tid % EC4) << 2;

  // ---- B: global fp32 -> registers -> split into LDS
  const LdsBLoad<BN> bload(a, g, k.n0, srow);
  constexpr int BV = LdsBLoad<BN>::BV;
  auto load_b = [&](int tap, int c0, f32x4 (&reg)[BV]) { bload.load(k.W + (long long)tap * a.w_ts, c0, reg); };
  auto store_b = [&](char* Bs, const f32x4 (&reg)[BV]) {
#pragma unroll
    for (int v = 0; v < BV; ++v) put_split4(Bs + (32 * v + srow) * ERS, c4, reg[v]);
  };

  // ---- A (halo convs): one chunk's nrows_a x 32 tile, pre-activation and row mask applied, split into LDS
  auto stage_a = [&](char* As, int c0) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if constexpr (!TWO_D) {
      // a thread keeps one 4-channel column and walks rows NT / EC4 apart: constant address steps
      constexpr int RSTEP = NT / EC4;
      const int c = c0 + c4;
      const bool cv = g.vec_a && c + 4 <= a.C_in;
      int r = tid / EC4;
      const float* src = k.X + (long long)(k.row0 + r) * a.ldx + c;
      const long long src_step = (long long)RSTEP * a.ldx;
      for (; r < g.nrows_a; r += RSTEP, src += src_step) {
        long long row;
        const bool ok = lds_src_row<false>(a, k, r, row) && c < a.C_in;
        put_split4(As + r * ERS, c4, ok ? lds_stage4(a, k, src, c, row, cv) : zero);
      }
    } else {
      for (int idx = tid; idx < g.nrows_a * EC4; idx += NT) {
        const int r = idx / EC4;
        const int c = c0 + c4;
        const bool cv = g.vec_a && c + 4 <= a.C_in;
        long long row;
        const bool ok = lds_src_row<true>(a, k, r, row) && c < a.C_in;
        put_split4(As + r * ERS, c4, ok ? lds_stage4(a, k, k.X + row * a.ldx + c, c, row, cv) : zero);
      }
    }
  };

  // ---- A (1-D): register prefetch of a whole chunk tile, issued one chunk ahead and written (split) at the chunk
  // change; tiles up to BM + 64 rows (every halo conv of the path but HuBERT's strided feature convs)
  // 2-D (the (rh + KH - 1) x (rw + KW - 1) pixel window) measured slower with the prefetch (U-Net 64x64 convs
  // 2.58 vs 2.47 ms per C2 step: 134 vs 105 VGPRs), so 2-D tiles stage synchronously
  constexpr int AP = ((BM + 64) * EC4 + NT - 1) / NT;
  f32x4 apre[AP];
  float apm[AP];  // 0 outside the input, else the row mask
  const bool a_pre = !PIPE && !TWO_D && g.nrows_a * EC4 <= AP * NT;
  const bool a_fast = g.vec_a && (a.C_in % EK) == 0;  // uniform: every slot's load is one vector
  auto load_a_regs = [&](int c0) {
    const int c = c0 + c4;
#pragma unroll
    for (int v = 0; v < AP; ++v) {
      const int r = v * (NT / EC4) + srow;
      long long row;
      apre[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      apm[v] = 0.f;
      if (lds_src_row<false>(a, k, r, row) && r < g.nrows_a) {
        apre[v] = lds_load4(k.X + row * a.ldx + c, c, a.C_in, a_fast);
        apm[v] = lds_row_mask(k, row);
      }
    }
  };
  auto write_a_regs = [&](char* As) {
#pragma unroll
    for (int v = 0; v < AP; ++v) {
      const int r = v * (NT / EC4) + srow;
      // times 0 outside the input (every activation is finite at 0), the row mask inside
      if (r < g.nrows_a) put_split4(As + r * ERS, c4, lds_pre4(a, apre[v], apm[v], true));
    }
  };

  // ---- MFMA: 2 K16 steps x 6 plane products, smallest terms first
  auto compute = [&](const char* As, const char* Bs, int tap) {
    const int toff = lds_tap_row<TWO_D>(a, k, tap) * ERS;
    // every fragment of both K16 steps is requested before the first MFMA: one exposed LDS latency per tap
    bf16x8 af[2][3], bfr[2][3];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        af[s][q] = *reinterpret_cast<const bf16x8*>(As + aoff + toff + q * PLANE + s * 32);
        bfr[s][q] = *reinterpret_cast<const bf16x8*>(Bs + boff + q * PLANE + s * 32);
      }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][2], bfr[s][0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][1], bfr[s][1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][0], bfr[s][2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][1], bfr[s][0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][0], bfr[s][1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s][0], bfr[s][0], acc, 0, 0, 0);
    }
  };

  const int nchunks = (a.C_in + EK - 1) / EK;
  f32x4 breg[BV];
  int it0, it1;
  if constexpr (!PIPE) {
    // (chunk, tap) iterations of this split-K slice; B of the next iteration is in flight during the MFMAs
    lds_slice(g, k, nchunks * a.taps, it0, it1);
    if (it0 < it1) {
      int ch = it0 / a.taps, tap = it0 - ch * a.taps;
      load_b(tap, ch * EK, breg);
      if (a_pre) {
        load_a_regs(ch * EK);
        write_a_regs(A0);
        if ((ch + 1) * a.taps < it1) load_a_regs((ch + 1) * EK);  // in flight across this chunk's taps
      } else {
        stage_a(A0, ch * EK);
      }
      store_b(B0, breg);
      __syncthreads();
      bool odd = false;
      for (int it = it0; it < it1; ++it) {
        const bool more = it + 1 < it1;
        int nch = ch, ntap = tap + 1;
        if (ntap == a.taps) {
          ntap = 0;
          ++nch;
        }
        if (more) load_b(ntap, nch * EK, breg);
        compute(A0, odd ? B1 : B0, tap);
        if (more) {
          if (nch != ch) {
            __syncthreads();  // every wave is done with this chunk's A tile
            if (a_pre) {
              write_a_regs(A0);
              if ((nch + 1) * a.taps < it1) load_a_regs((nch + 1) * EK);
            } else {
              stage_a(A0, nch * EK);
            }
          }
          store_b(odd ? B0 : B1, breg);
          __syncthreads();
          odd = !odd;
        }
        ch = nch;
        tap = ntap;
      }
    }
  } else {
    // plain GEMM: A and B both double buffered, the next chunk's tiles in registers during the MFMAs
    constexpr int AV = BM * EC4 / NT;
    f32x4 areg[AV];
    float amk[AV];  // 0 outside the input, else the row mask
    auto load_a = [&](int c0) {
      const int c = c0 + c4;
      const bool cv = g.vec_a && c + 4 <= a.C_in;
#pragma unroll
      for (int v = 0; v < AV; ++v) {
        long long row;
        areg[v] = f32x4{0.f, 0.f, 0.f, 0.f};
        amk[v] = 0.f;
        if (lds_src_row<false>(a, k, v * (NT / EC4) + tid / EC4, row) && c < a.C_in) {
          amk[v] = lds_row_mask(k, row);
          areg[v] = lds_load4(k.X + row * a.ldx + c, c, a.C_in, cv);
        }
      }
    };
    auto store_a = [&](char* dst) {
#pragma unroll
      for (int v = 0; v < AV; ++v) {
        const f32x4 val = amk[v] != 0.f ? lds_pre4(a, areg[v], amk[v], k.PM != nullptr) : f32x4{0.f, 0.f, 0.f, 0.f};
        put_split4(dst + (v * (NT / EC4) + tid / EC4) * ERS, c4, val);
      }
    };
    lds_slice(g, k, nchunks, it0, it1);
    if (it0 < it1) {
      load_a(it0 * EK);
      load_b(0, it0 * EK, breg);
      store_a(A0);
      store_b(B0, breg);
      __syncthreads();
      for (int it = it0; it < it1; ++it) {
        const bool odd = (it - it0) & 1;
        const bool more = it + 1 < it1;
        if (more) {
          load_a((it + 1) * EK);
          load_b(0, (it + 1) * EK, breg);
        }
        compute(odd ? A1 : A0, odd ? B1 : B0, 0);
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

template <int BM, int BN, int WM, int WN, bool TWO_D, bool PIPE>
hipError_t launch_emu(const ConvArgs& a, int ksplit, hipStream_t s) {
  if (PIPE && (a.taps != 1 || a.stride != 1)) return hipErrorInvalidValue;
  const LdsGeom g(a, BM, BN, TWO_D, ksplit);
  static size_t lds_set = LDS_SET0;
  return g.launch(conv_emu_kernel<BM, BN, WM, WN, TWO_D, PIPE>, lds_set, a,
                  (size_t)(PIPE ? 2 * (BM + BN) : g.nrows_a + 2 * BN) * ERS, s);
}

template <int BM, int BN, int WM, int WN>
hipError_t launch_tile(const ConvArgs& a, bool two_d, bool pipe, int ksplit, hipStream_t s) {
  if (two_d) return pipe ? hipErrorInvalidValue : launch_emu<BM, BN, WM, WN, true, false>(a, ksplit, s);
  return pipe ? launch_emu<BM, BN, WM, WN, false, true>(a, ksplit, s)
              : launch_emu<BM, BN, WM, WN, false, false>(a, ksplit, s);
}

}  // namespace

// a split launch (ksplit > 1) leaves the combine to the caller; hipErrorInvalidValue: the tile's LDS does not fit, the
// tile is not this family's, or it has no such form
hipError_t conv_emu_launch(const ConvArgs& a, int cfg, bool two_d, bool pipe, int ksplit, hipStream_t s) {
  switch (cfg) {
    case TILE_EMU_128x32: return launch_tile<128, 32, 4, 1>(a, two_d, pipe, ksplit, s);
    case TILE_EMU_64x64: return launch_tile<64, 64, 2, 2>(a, two_d, pipe, ksplit, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace rvcx
