// Implicit-GEMM convolution on CDNA4 fp32 MFMA (v_mfma_f32_32x32x2_f32).
//
// One kernel family covers every contraction of the RVC path:
//   * 1-D conv (time-major [T][C]): NSF ResBlock dilated convs, conv_pre, flow WaveNet,
//     TextEncoder FFN, HuBERT strided feature convs, the grouped positional conv (batch=group),
//     ConvTranspose1d as a polyphase conv (u*C_out virtual outputs), STFT-as-GEMM framing;
//   * GEMM (taps=1): all Linear / 1x1 convs, attention QK^T and PV (batch = head);
//   * 2-D 3x3 conv on NHWC images (RMVPE U-Net), ConvTranspose2d as a 2x2-tap phase conv.
//
// Tiling: a 256-thread block (4 waves) owns BM output rows x BN output channels. The A tile is
// staged once per 32-channel chunk with its full tap halo ((BM-1)*stride + (taps-1)*dil + 1 rows,
// or the (RH+KH-1) x (RW+KW-1) pixel window in 2-D), the pre-activation applied on the way into
// LDS; each tap then re-reads shifted rows of that tile (no im2col in HBM). B (weights packed
// [tap][N][C]) is staged per tap. Each wave holds TM x TN 32x32 fp32 accumulators; one
// ds_read_b128 per operand feeds 4 MFMAs (the k-pair of MFMA j is channels {8kk+j, 8kk+4+j}).
// fp32 in / fp32 accumulate MFMA is a bit-exact fp32 fma chain at the FP32 vector peak rate.
#include <algorithm>

#include "conv_common.h"

namespace rvcx {

constexpr int CK = 32;   // contraction channels per LDS chunk
constexpr int NTHREADS = CONV_THREADS;

template <int BM, int BN, int WM, int WN, bool TWO_D, bool PIPE, int ASB, int CKT = CK>
__global__ __launch_bounds__(NTHREADS, 2) void conv_gemm_kernel(const ConvArgs a, const int nrows_a, const int rw,
                                                             const int rh, const int tiles_w, const int vec_a,
                                                             const int vec_b, const int ksplit, const int ntn) {
  constexpr int CKP = CKT + 4;  // padded LDS row: rows i..i+15 land on distinct 16-B bank slots
  constexpr int C4 = CKT / 4;   // float4 per LDS row
  constexpr int TM = BM / (WM * 32);
  constexpr int TN = BN / (WN * 32);
  static_assert(WM * WN == 4, "4 waves per block");
  static_assert(TM >= 1 && TN >= 1, "tile too small");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;
  float* Bs0 = smem + nrows_a * CKP;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, hk = lane >> 5;
  // Tile order (ntn > 0): the grid is 1-D over (M tile, N tile) with N fastest, and the linear workgroup
  // id is remapped so each XCD (workgroups are dealt to the 8 XCDs round-robin) owns one contiguous run of
  // tiles: the N tiles of an M tile then share its A halo through one L2 instead of re-reading it from
  // HBM/L3 (bijective remap, cdna_hip_programming.md T1). ntn = 0: the plain (x = M, y = N) grid.
  int bx, by, bz;
  conv_block_coords(ntn, bx, by, bz);
  const int zsplit = bz % ksplit;     // split-K slice
  const int zb = bz / ksplit;
  const int b = zb / a.batch_inner;   // outer batch
  const int bi = zb % a.batch_inner;  // inner batch (heads / groups)
  const int n0 = by * BN;
  int m0 = 0, h0 = 0, w0 = 0;
  if (!TWO_D) {
    m0 = bx * BM;
  } else {
    h0 = (bx / tiles_w) * rh;
    w0 = (bx % tiles_w) * rw;
  }
  const float* X = a.x + (long long)b * a.x_bs + (long long)bi * a.x_bs2;
  const float* Wb = a.w + (long long)b * a.w_bs + (long long)bi * a.w_bs2;
  const float* PM = a.pre_mask ? a.pre_mask + (long long)b * a.pre_mask_bs : nullptr;
  const int Hi = TWO_D ? conv_rows_in(a, b) : a.T_in;  // 2-D: the image's own rows (ConvArgs::h_in)
  const int aw = TWO_D ? rw + a.KW - 1 : 0;
  const int row0 = TWO_D ? 0 : m0 * a.stride - a.pad;

  int base[TM];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int ml = wm * TM * 32 + tm * 32 + li;
    if (!TWO_D) {
      base[tm] = ml * a.stride;
    } else {
      base[tm] = (ml < rh * rw) ? (ml / rw) * aw + (ml % rw) : 0;
    }
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

  // B tile loader: global -> registers (BN x 32 floats of (tap, chunk)); NK or KN weight layout
  constexpr int BV = (BN * C4 + NTHREADS - 1) / NTHREADS;  // float4 per thread
  // NK layout: thread v-slot reads row n0 + idx / C4, channels c0 + 4 (idx % C4): the row offset is fixed for
  // the whole kernel, so it is computed once (32-bit: one layer's weights are < 2^31 floats)
  int b_row_off[BV];
  bool b_row_ok[BV];
#pragma unroll
  for (int v = 0; v < BV; ++v) {
    const int idx = tid + v * NTHREADS;
    const int gn = n0 + idx / C4;
    b_row_ok[v] = idx < BN * C4 && gn < a.N;
    b_row_off[v] = gn * a.ldw + ((idx % C4) << 2);
  }
  auto load_b = [&](int tap, int c0, f32x4 (&reg)[BV]) {
    const float* Wt = Wb + (long long)tap * a.w_ts;
#pragma unroll
    for (int v = 0; v < BV; ++v) {
      const int idx = tid + v * NTHREADS;
      f32x4 val = {0.f, 0.f, 0.f, 0.f};
      if (idx < BN * C4) {
        if (!a.b_kn) {
          const int c = c0 + ((idx % C4) << 2);
          if (b_row_ok[v] && c < a.C_in) {
            const float* src = Wt + c0 + b_row_off[v];
            if (vec_b && c + 4 <= a.C_in) {
              val = *reinterpret_cast<const f32x4*>(src);
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j) val[j] = (c + j < a.C_in) ? src[j] : 0.f;
            }
          }
        } else {
          const int cc = idx / (BN / 4);
          const int n4 = (idx - cc * (BN / 4)) << 2;
          const int gc = c0 + cc, gn = n0 + n4;
          if (gc < a.C_in && gn < a.N) {
            const float* src = Wt + (long long)gc * a.ldw + gn;
            if (vec_b && gn + 4 <= a.N) {
              val = *reinterpret_cast<const f32x4*>(src);
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j) val[j] = (gn + j < a.N) ? src[j] : 0.f;
            }
          }
        }
      }
      reg[v] = val;
    }
  };
  auto store_b = [&](float* Bs, const f32x4 (&reg)[BV]) {
#pragma unroll
    for (int v = 0; v < BV; ++v) {
      const int idx = tid + v * NTHREADS;
      if (idx < BN * C4) {
        if (!a.b_kn) {
          *reinterpret_cast<f32x4*>(&Bs[(idx / C4) * CKP + ((idx % C4) << 2)]) = reg[v];
        } else {
          const int cc = idx / (BN / 4);
          const int n4 = (idx - cc * (BN / 4)) << 2;
#pragma unroll
          for (int j = 0; j < 4; ++j) Bs[(n4 + j) * CKP + cc] = reg[v][j];
        }
      }
    }
  };
  // A tile: nrows_a x 32 channels of chunk c0 -> LDS, pre-activation applied, zero outside the input
  auto stage_a_serial = [&](int c0) {
    if constexpr (!TWO_D) {
      // 1-D: a thread keeps one 4-channel column and walks rows NTHREADS / C4 apart, so the source and LDS
      // addresses advance by constants (no per-element 64-bit index math)
      constexpr int RSTEP = NTHREADS / C4;
      const int c4 = (tid % C4) << 2;
      const int c = c0 + c4;
      const bool c_ok = c < a.C_in;
      const bool c_vec = vec_a && c + 4 <= a.C_in;
      int r = tid / C4;
      int g = row0 + r;
      const float* src = X + (long long)g * a.ldx + c;
      const long long src_step = (long long)RSTEP * a.ldx;
      for (; r < nrows_a; r += RSTEP, g += RSTEP, src += src_step) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (c_ok && g >= 0 && g < a.T_in) {
          if (c_vec) {
            v = *reinterpret_cast<const f32x4*>(src);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (c + j < a.C_in) ? src[j] : 0.f;
          }
          if (a.pre_act != ACT_NONE) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = act_fn(v[j], a.pre_act, a.pre_slope);
          }
          if (PM) {
            const float mk = PM[g];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= mk;
          }
        }
        *reinterpret_cast<f32x4*>(&As[r * CKP + c4]) = v;
      }
      return;
    }
    for (int idx = tid; idx < nrows_a * C4; idx += NTHREADS) {
      const int r = idx / C4;
      const int c4 = (idx % C4) << 2;
      const int c = c0 + c4;
      long long grow;
      bool valid;
      if (!TWO_D) {
        const int g = row0 + r;
        valid = (g >= 0) && (g < a.T_in);
        grow = g;
      } else {
        const int ah = r / aw, awi = r - ah * aw;
        const int gh = h0 - a.padh + ah, gw = w0 - a.padw + awi;
        valid = (gh >= 0) && (gh < Hi) && (gw >= 0) && (gw < a.W_in);
        grow = (long long)gh * a.W_in + gw;
      }
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (valid && c < a.C_in) {
        const float* src = X + grow * a.ldx + c;
        if (vec_a && c + 4 <= a.C_in) {
          v = *reinterpret_cast<const f32x4*>(src);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = (c + j < a.C_in) ? src[j] : 0.f;
        }
        if (a.pre_act != ACT_NONE) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = act_fn(v[j], a.pre_act, a.pre_slope);
        }
        if (PM) {
          const float mk = PM[grow];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] *= mk;
        }
      }
      *reinterpret_cast<f32x4*>(&As[r * CKP + c4]) = v;
    }
  };
  // batched staging: ASB float4 loads per thread in flight before the first wait, then the transform
  auto stage_a = [&](int c0) {
    if constexpr (ASB <= 1) {
      stage_a_serial(c0);
    } else {
      const int total = nrows_a * C4;
      for (int base = 0; base < total; base += ASB * NTHREADS) {
        f32x4 rv[ASB];
        float mk[ASB];
#pragma unroll
        for (int q = 0; q < ASB; ++q) {
          const int idx = base + tid + q * NTHREADS;
          rv[q] = f32x4{0.f, 0.f, 0.f, 0.f};
          mk[q] = 0.f;
          if (idx < total) {
            const int r = idx / C4;
            const int c = c0 + ((idx % C4) << 2);
            long long grow;
            bool valid;
            if (!TWO_D) {
              const int g = row0 + r;
              valid = (g >= 0) && (g < a.T_in);
              grow = g;
            } else {
              const int ah = r / aw, awi = r - ah * aw;
              const int gh = h0 - a.padh + ah, gw = w0 - a.padw + awi;
              valid = (gh >= 0) && (gh < Hi) && (gw >= 0) && (gw < a.W_in);
              grow = (long long)gh * a.W_in + gw;
            }
            if (valid && c < a.C_in) {
              mk[q] = PM ? PM[grow] : 1.f;
              const float* src = X + grow * a.ldx + c;
              if (vec_a && c + 4 <= a.C_in) {
                rv[q] = *reinterpret_cast<const f32x4*>(src);
              } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) rv[q][j] = (c + j < a.C_in) ? src[j] : 0.f;
              }
            }
          }
        }
#pragma unroll
        for (int q = 0; q < ASB; ++q) {
          const int idx = base + tid + q * NTHREADS;
          if (idx < total) {
            f32x4 v = rv[q];
            if (mk[q] != 0.f) {
              if (a.pre_act != ACT_NONE) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = act_fn(v[j], a.pre_act, a.pre_slope);
              }
              if (PM) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] *= mk[q];
              }
            } else {
              v = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            *reinterpret_cast<f32x4*>(&As[(idx / C4) * CKP + ((idx % C4) << 2)]) = v;
          }
        }
      }
    }
  };
  auto compute = [&](const float* Bs, int tap) {
    const int toff = TWO_D ? (tap / a.KW) * aw + (tap % a.KW) : tap * a.dil;
#pragma unroll
    for (int kk = 0; kk < CKT; kk += 8) {
      float av[TM][4], bv[TN][4];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(&As[(base[tm] + toff) * CKP + kk + hk * 4]);
        av[tm][0] = t[0]; av[tm][1] = t[1]; av[tm][2] = t[2]; av[tm][3] = t[3];
      }
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(&Bs[(wn * TN * 32 + tn * 32 + li) * CKP + kk + hk * 4]);
        bv[tn][0] = t[0]; bv[tn][1] = t[1]; bv[tn][2] = t[2]; bv[tn][3] = t[3];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm][j], bv[tn][j], acc[tm][tn], 0, 0, 0);
    }
  };

  const int nchunks = (a.C_in + CKT - 1) / CKT;
  if (!PIPE) {
    f32x4 breg[BV];
    const int total = nchunks * a.taps;
    const int per = (total + ksplit - 1) / ksplit;
    const int it0 = zsplit * per, it1 = min(total, it0 + per);
    int it = it0;
    while (it < it1) {
      const int ch = it / a.taps;
      __syncthreads();
      stage_a(ch * CKT);
      for (int tap = it - ch * a.taps; tap < a.taps && it < it1; ++tap, ++it) {
        if (it > it0 && tap != it0 - ch * a.taps) __syncthreads();
        load_b(tap, ch * CKT, breg);
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
    constexpr int AV = (BM * C4 + NTHREADS - 1) / NTHREADS;
    float* const A0 = smem;
    float* const A1 = smem + BM * CKP;
    float* const B0 = smem + 2 * BM * CKP;
    float* const B1 = B0 + BN * CKP;
    f32x4 areg[AV];
    float amk[AV];
    f32x4 breg[BV];
    auto load_a = [&](int c0) {
#pragma unroll
      for (int v = 0; v < AV; ++v) {
        const int idx = tid + v * NTHREADS;
        areg[v] = f32x4{0.f, 0.f, 0.f, 0.f};
        amk[v] = 0.f;
        if (idx < BM * C4) {
          const int r = idx / C4;
          const int c = c0 + ((idx % C4) << 2);
          const int g = row0 + r;
          if (g >= 0 && g < a.T_in && c < a.C_in) {
            amk[v] = PM ? PM[g] : 1.f;
            const float* src = X + (long long)g * a.ldx + c;
            if (vec_a && c + 4 <= a.C_in) {
              areg[v] = *reinterpret_cast<const f32x4*>(src);
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j) areg[v][j] = (c + j < a.C_in) ? src[j] : 0.f;
            }
          }
        }
      }
    };
    auto store_a = [&](float* dst) {
#pragma unroll
      for (int v = 0; v < AV; ++v) {
        const int idx = tid + v * NTHREADS;
        if (idx < BM * C4) {
          f32x4 val = areg[v];
          if (amk[v] != 0.f) {
            if (a.pre_act != ACT_NONE) {
#pragma unroll
              for (int j = 0; j < 4; ++j) val[j] = act_fn(val[j], a.pre_act, a.pre_slope);
            }
            if (PM) {
#pragma unroll
              for (int j = 0; j < 4; ++j) val[j] *= amk[v];
            }
          } else {
            val = f32x4{0.f, 0.f, 0.f, 0.f};
          }
          *reinterpret_cast<f32x4*>(&dst[(idx / C4) * CKP + ((idx % C4) << 2)]) = val;
        }
      }
    };
    const int per = (nchunks + ksplit - 1) / ksplit;
    const int it0 = zsplit * per, it1 = min(nchunks, it0 + per);
    if (it0 < it1) {
      load_a(it0 * CKT);
      load_b(0, it0 * CKT, breg);
      store_a(A0);
      store_b(B0, breg);
      __syncthreads();
      for (int it = it0; it < it1; ++it) {
        const bool odd = (it - it0) & 1;
        const bool more = it + 1 < it1;
        if (more) {
          load_a((it + 1) * CKT);
          load_b(0, (it + 1) * CKT, breg);
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

  // ---- epilogue
  conv_store_tile<TM, TN, WM, WN, TWO_D>(a, TilePos{m0, h0, w0, rw, rh, n0, b, bi, zb, zsplit, ksplit}, acc, smem);
}

namespace {

template <int BM, int BN, int WM, int WN, bool TWO_D, bool PIPE = false, int ASB = 1, int CKT = CK>
hipError_t launch_cfg(const ConvArgs& a, int ksplit, hipStream_t s) {
  constexpr int CKP = CKT + 4;
  int nrows_a, rw = 0, rh = 0, tiles_w = 1, mtiles;
  if (!TWO_D) {
    nrows_a = (BM - 1) * a.stride + (a.taps - 1) * a.dil + 1;
    mtiles = (a.T_out + BM - 1) / BM;
  } else {
    rw = a.W_out < BM ? a.W_out : BM;
    rh = BM / rw;
    tiles_w = (a.W_out + rw - 1) / rw;
    mtiles = ((a.T_out + rh - 1) / rh) * tiles_w;
    nrows_a = (rh + a.KH - 1) * (rw + a.KW - 1);
  }
  if (PIPE && (TWO_D || a.taps != 1 || a.stride != 1)) return hipErrorInvalidValue;
  size_t smem = (size_t)(PIPE ? 2 : 1) * (nrows_a + BN) * CKP * sizeof(float);
  smem = std::max(smem, (size_t)4 * 32 * 33 * sizeof(float));  // epilogue staging slots (2x2-per-wave tiles)
  if (smem > 160 * 1024) return hipErrorInvalidValue;
  const int vec_a = ((a.ldx & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.x) & 15) == 0) &&
                    ((a.x_bs & 3) == 0) && ((a.x_bs2 & 3) == 0);
  const int vec_b = ((a.ldw & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.w) & 15) == 0) &&
                    ((a.w_bs & 3) == 0) && ((a.w_bs2 & 3) == 0) && ((a.w_ts & 3) == 0);
  if (a.batch_inner < 1) return hipErrorInvalidValue;
  const int ntiles = (a.N + BN - 1) / BN;
  const int ntn = ntiles;  // XCD-contiguous tile runs (conv_block_coords)
  dim3 grid(mtiles * ntiles, 1, a.batch * a.batch_inner * ksplit);
  auto kern = conv_gemm_kernel<BM, BN, WM, WN, TWO_D, PIPE, ASB, CKT>;
  static size_t smem_set = 64 * 1024;  // per instantiation: raise the dynamic-LDS limit once, not per launch
  if (smem > smem_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    smem_set = smem;
  }
  hipLaunchKernelGGL(kern, grid, dim3(NTHREADS), smem, s, a, nrows_a, rw, rh, tiles_w, vec_a, vec_b, ksplit, ntn);
  return hipGetLastError();
}

template <bool TWO_D, bool PIPE, int ASB>
hipError_t launch_tile(const ConvArgs& a, int cfg, int ksplit, hipStream_t s) {
  switch (cfg) {
    case 0: return launch_cfg<256, 32, 4, 1, TWO_D, PIPE, ASB>(a, ksplit, s);
    case 1: return launch_cfg<128, 32, 4, 1, TWO_D, PIPE, ASB>(a, ksplit, s);
    case 2: return launch_cfg<128, 64, 2, 2, TWO_D, PIPE, ASB>(a, ksplit, s);
    case 3: return launch_cfg<64, 64, 2, 2, TWO_D, PIPE, ASB>(a, ksplit, s);
    case 4: return launch_cfg<128, 128, 2, 2, TWO_D, PIPE, ASB>(a, ksplit, s);
    case 5: return launch_cfg<64, 128, 2, 2, TWO_D, PIPE, ASB>(a, ksplit, s);
    case 6: return launch_cfg<256, 64, 4, 1, TWO_D, PIPE, ASB>(a, ksplit, s);
    case 7: return launch_cfg<64, 64, 2, 2, TWO_D, PIPE, ASB, 64>(a, ksplit, s);
    case 8: return launch_cfg<128, 32, 4, 1, TWO_D, PIPE, ASB, 64>(a, ksplit, s);
    case 9: return launch_cfg<128, 128, 2, 2, TWO_D, PIPE, ASB, 64>(a, ksplit, s);
    default: return hipErrorInvalidValue;
  }
}

// A-tile staging: serial (1, the default) or 4 loads in flight per thread (ConvArgs::astage = 4)
template <bool TWO_D>
hipError_t launch_staged(const ConvArgs& a, int cfg, bool pipe, int ksplit, hipStream_t s) {
  const int asb = a.astage > 0 ? a.astage : 1;
  if (!pipe && asb >= 4) return launch_tile<TWO_D, false, 4>(a, cfg, ksplit, s);
  return pipe ? launch_tile<TWO_D, true, 1>(a, cfg, ksplit, s) : launch_tile<TWO_D, false, 1>(a, cfg, ksplit, s);
}

}  // namespace

// cfg 0..9 (cfg_tile); a split launch (ksplit > 1) leaves the combine to the caller, as conv_emu_launch does; returns
// hipErrorInvalidValue when the tile's LDS does not fit or the tile has no such form
hipError_t conv_gemm_launch(const ConvArgs& a, int cfg, bool two_d, bool pipe, int ksplit, hipStream_t s) {
  return two_d ? launch_staged<true>(a, cfg, pipe, ksplit, s) : launch_staged<false>(a, cfg, pipe, ksplit, s);
}

}  // namespace rvcx
