// The one-thread-per-output conv kernels for contractions far shorter than an MFMA chunk, the shapes they take
// (*_fits) and their launchers.
#include <algorithm>

#include "conv_common.h"

namespace rvcx {

// Contractions far shorter than one 32-channel MFMA chunk (C_in <= 4 and at most 16 MACs per output: RMVPE's 3x3
// and 1x1 convs on the 1-channel mel image, the generator's last 1-tap noise conv) would run the MFMA tile on
// >= 87 % zero padding: one thread per output element instead, an fp32 fma chain over (tap, channel), then the
// shared epilogue. (The long-tap C_in = 1 noise convs stay on the MFMA kernel: 80 dependent loads per output
// measured 351 vs 110 us.) Outputs are n-fastest,
// so stores and weight reads coalesce and a thread group shares its input rows through L1.
template <bool TWO_D>
__global__ void conv_tiny_kernel(const ConvArgs a) {
  // 32-bit index math (launch_tiny checks the sizes): one output element per thread, n fastest
  const int rows = TWO_D ? a.T_out * a.W_out : a.T_out;
  const int per_b = rows * a.N;
  const int total = per_b * a.batch * a.batch_inner;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int zb = i / per_b;
    const int rem = i - zb * per_b;
    const int m = rem / a.N;
    const int n = rem - m * a.N;
    const int b = zb / a.batch_inner, bi = zb - (zb / a.batch_inner) * a.batch_inner;
    const float* X = a.x + (long long)b * a.x_bs + (long long)bi * a.x_bs2;
    const float* Wb = a.w + (long long)b * a.w_bs + (long long)bi * a.w_bs2;
    const float* PM = a.pre_mask ? a.pre_mask + (long long)b * a.pre_mask_bs : nullptr;
    int oh = 0, ow = 0;
    if (TWO_D) {
      oh = m / a.W_out;
      ow = m - oh * a.W_out;
    }
    // the image's own rows (ConvArgs::h_in; launch_tiny admits it where a wave's 64 outputs lie in one image)
    const int Hi = (TWO_D && a.h_in) ? conv_rows_in(a, __builtin_amdgcn_readfirstlane(b)) : a.T_in;
    float acc = 0.f;
    for (int tap = 0; tap < a.taps; ++tap) {
      int g;
      if (!TWO_D) {
        g = m * a.stride - a.pad + tap * a.dil;
        if (g < 0 || g >= a.T_in) continue;
      } else {
        const int kh = tap / a.KW;
        const int gh = oh - a.padh + kh, gw = ow - a.padw + (tap - kh * a.KW);
        if (gh < 0 || gh >= Hi || gw < 0 || gw >= a.W_in) continue;
        g = gh * a.W_in + gw;
      }
      const float pm = (PM && !TWO_D) ? PM[g] : 1.f;
      const float* Wt = Wb + (long long)tap * a.w_ts;
      for (int c = 0; c < a.C_in; ++c) {
        const float v = act_fn(X[(long long)g * a.ldx + c], a.pre_act, a.pre_slope) * pm;
        const float wv = Wt[(long long)n * a.ldw + c];
        acc = fmaf(v, wv, acc);
      }
    }
    const EpiPtrs e = epi_ptrs(a, b, bi);
    epilogue_store(a, acc, e.bias ? e.bias[n] : 0.f, m, n, oh, ow, e);
  }
}

// The tiny contractions whose epilogue is only bias + activation + store (the RMVPE U-Net's first ConvBlockRes on the
// 1-channel mel image: the 3x3 1 -> 16 conv and the 1x1 shortcut), one thread per output ROW computing all N <= 32
// outputs: the weights and bias in LDS, the <= 16 inputs read once instead of once per output, the activation a
// compile-time choice, float4 stores. (conv_tiny_kernel's per-element index math, activation switch and shared epilogue
// took 100-135 us for these two 3.2 M-output convs.)
template <bool TWO_D, int N, int ACT>
__global__ __launch_bounds__(256) void conv_tiny_rows_kernel(const ConvArgs a) {
  __shared__ float ws[16 * 32], bs[32];
  const int ck = a.C_in * a.taps;  // <= 16
  for (int i = threadIdx.x; i < ck * N; i += blockDim.x) {
    const int tap = i / (a.C_in * N), r = i - tap * (a.C_in * N);
    const int n = r / a.C_in, c = r - n * a.C_in;
    ws[(tap * a.C_in + c) * N + n] = a.w[(long long)tap * a.w_ts + (long long)n * a.ldw + c];
  }
  if (threadIdx.x < N) bs[threadIdx.x] = a.bias ? a.bias[threadIdx.x] : 0.f;
  __syncthreads();
  const int rows = TWO_D ? a.T_out * a.W_out : a.T_out;
  const int total = rows * a.batch;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / rows, m = i - b * rows;
    const float* X = a.x + (long long)b * a.x_bs;
    float acc[N];
#pragma unroll
    for (int n = 0; n < N; ++n) acc[n] = 0.f;
    int oh = 0, ow = m;
    if (TWO_D) {
      oh = m / a.W_out;
      ow = m - oh * a.W_out;
    }
    const int Hi = (TWO_D && a.h_in) ? conv_rows_in(a, __builtin_amdgcn_readfirstlane(b)) : a.T_in;  // as conv_tiny_kernel
    for (int tap = 0; tap < a.taps; ++tap) {
      int g;
      if (!TWO_D) {
        g = m * a.stride - a.pad + tap * a.dil;
        if (g < 0 || g >= a.T_in) continue;
      } else {
        const int kh = tap / a.KW;
        const int gh = oh - a.padh + kh, gw = ow - a.padw + (tap - kh * a.KW);
        if (gh < 0 || gh >= Hi || gw < 0 || gw >= a.W_in) continue;
        g = gh * a.W_in + gw;
      }
      for (int c = 0; c < a.C_in; ++c) {
        const float v = X[(long long)g * a.ldx + c];
        const float* wr = ws + (tap * a.C_in + c) * N;
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = fmaf(v, wr[n], acc[n]);
      }
    }
    float* Y = a.y + (long long)b * a.y_bs + (long long)m * a.ldy;
#pragma unroll
    for (int n = 0; n < N; n += 4) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[n + e] + bs[n + e];  // conv_tiny_kernel's order: the fma chain, then the bias
        if (ACT == ACT_RELU) v = v > 0.f ? v : 0.f;
        else if (ACT == ACT_LRELU) v = v > 0.f ? v : v * a.slope;
        o[e] = v;
      }
      *reinterpret_cast<f32x4*>(Y + n) = o;
    }
  }
}

// 1x1 convs with few inputs and outputs (the U-Net's ConvBlockRes shortcuts: 16 -> 32, 64 -> 32, 32 -> 16 channels on
// 50 k - 200 k pixels; round 5): one thread per pixel, its C_in inputs as float4 loads, the weights [C_in][N] and bias in
// LDS (broadcast reads), N fp32 fma chains, bias + activation, float4 stores. Exact fp32 (the native-f32 MFMA GEMM it
// replaces took 13-23 us for these byte-bound shapes).
template <int N, int ACT>
__global__ __launch_bounds__(256) void conv_rows1x1_kernel(const ConvArgs a) {
  // (staging the block's input rows through LDS for coalesced loads measured slower: 16 / 20 us vs 12 / 18, r05aq)
  __shared__ __attribute__((aligned(16))) float ws[64 * 32];
  __shared__ float bs[32];
  const int C = a.C_in;
  for (int i = threadIdx.x; i < C * N; i += blockDim.x) {
    const int n = i / C, c = i - n * C;
    ws[c * N + n] = a.w[(long long)n * a.ldw + c];
  }
  if (threadIdx.x < N) bs[threadIdx.x] = a.bias ? a.bias[threadIdx.x] : 0.f;
  __syncthreads();
  const int rows = a.W_out > 0 ? a.T_out * a.W_out : a.T_out;
  const int total = rows * a.batch;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / rows, m = i - b * rows;
    const f32x4* X = reinterpret_cast<const f32x4*>(a.x + (long long)b * a.x_bs + (long long)m * a.ldx);
    float acc[N];
#pragma unroll
    for (int n = 0; n < N; ++n) acc[n] = 0.f;
    for (int c4 = 0; c4 < C / 4; ++c4) {
      const f32x4 v = X[c4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x4* wr = reinterpret_cast<const f32x4*>(ws + (4 * c4 + e) * N);
#pragma unroll
        for (int n4 = 0; n4 < N / 4; ++n4) {
          const f32x4 w = wr[n4];
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[4 * n4 + k] = fmaf(v[e], w[k], acc[4 * n4 + k]);
        }
      }
    }
    float* Y = a.y + (long long)b * a.y_bs + (long long)m * a.ldy;
#pragma unroll
    for (int n = 0; n < N; n += 4) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[n + e] + bs[n + e];
        if (ACT == ACT_RELU) v = v > 0.f ? v : 0.f;
        else if (ACT == ACT_LRELU) v = v > 0.f ? v : v * a.slope;
        o[e] = v;
      }
      *reinterpret_cast<f32x4*>(Y + n) = o;
    }
  }
}

namespace {

// conv_tiny_rows_kernel's shapes: only bias + activation in the epilogue, N in {16, 32}, 16-B aligned output rows
inline bool tiny_rows_fits(const ConvArgs& a) {
  return (a.N == 16 || a.N == 32) && a.pre_act == ACT_NONE && !a.pre_mask && a.batch_inner == 1 &&
         a.out_map == OUT_ROWS && a.res_mode == RES_NONE && !a.mask && a.acc_mode == ACC_STORE && a.alpha == 1.f &&
         (a.act == ACT_NONE || a.act == ACT_RELU || a.act == ACT_LRELU) && (a.ldy & 3) == 0 && (a.y_bs & 3) == 0 &&
         (reinterpret_cast<uintptr_t>(a.y) & 15) == 0 && a.gate_h == 0;
}

}  // namespace

constexpr int TINY_MAX_CIN = 4;
bool tiny_fits(const ConvArgs& a) {
  const long long rows = a.W_out > 0 ? (long long)a.T_out * a.W_out : a.T_out;
  return a.C_in <= TINY_MAX_CIN && a.C_in * a.taps <= 16 &&
         rows * a.N * a.batch * a.batch_inner < (1LL << 30);
}

// conv_rows1x1_kernel's shapes: a 1x1 / stride-1 conv (1-D or 2-D) with C_in a multiple of 4 up to 64, 16-B aligned
// input rows, and conv_tiny_rows_kernel's epilogue conditions
bool rows1x1_fits(const ConvArgs& a, bool two_d) {
  if (a.taps != 1 || a.stride != 1 || a.dil != 1 || a.pad != 0) return false;
  if (two_d && (a.KH != 1 || a.KW != 1 || a.padh != 0 || a.padw != 0 || a.T_in != a.T_out || a.W_in != a.W_out))
    return false;
  const long long rows = two_d ? (long long)a.T_out * a.W_out : a.T_out;
  return tiny_rows_fits(a) && a.C_in % 4 == 0 && a.C_in >= 4 && a.C_in <= 64 && (a.ldx & 3) == 0 &&
         (a.x_bs & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0 && rows * a.batch < (1LL << 31) - 65536LL * 256;
}

hipError_t launch_rows1x1(const ConvArgs& a, bool two_d, hipStream_t s) {
  const long long rows = two_d ? (long long)a.T_out * a.W_out : a.T_out;
  const unsigned nb = (unsigned)std::min<long long>((rows * a.batch + 255) / 256, 65536);
  ConvArgs b = a;
  if (!two_d) b.W_out = 0;
#define ROWS1(NN, AC) hipLaunchKernelGGL((conv_rows1x1_kernel<NN, AC>), dim3(nb), dim3(256), 0, s, b)
  const int act = a.act;
  if (a.N == 16) { if (act == ACT_RELU) ROWS1(16, ACT_RELU); else if (act == ACT_LRELU) ROWS1(16, ACT_LRELU); else ROWS1(16, ACT_NONE); }
  else { if (act == ACT_RELU) ROWS1(32, ACT_RELU); else if (act == ACT_LRELU) ROWS1(32, ACT_LRELU); else ROWS1(32, ACT_NONE); }
#undef ROWS1
  return hipGetLastError();
}

hipError_t launch_tiny(const ConvArgs& a, bool two_d, hipStream_t s) {
  const long long rows = two_d ? (long long)a.T_out * a.W_out : a.T_out;
  const long long total = rows * a.N * a.batch * a.batch_inner;
  if (total >= (1LL << 31) - 65536LL * 256) return hipErrorInvalidValue;  // 32-bit indexing in the kernel
  // per-image heights: the kernels read the bound of the wave's first output, so a wave may not straddle two images
  if (a.h_in && (!two_d || (tiny_rows_fits(a) ? rows : rows * a.N) % 64 != 0)) return hipErrorInvalidValue;
  if (tiny_rows_fits(a)) {
    const long long nr = total / a.N;
    const unsigned nbr = (unsigned)std::min<long long>((nr + 255) / 256, 65536);
#define TINY_ROWS(TD, NN, AC) hipLaunchKernelGGL((conv_tiny_rows_kernel<TD, NN, AC>), dim3(nbr), dim3(256), 0, s, a)
    const int act = a.act;
    if (two_d) {
      if (a.N == 16) { if (act == ACT_RELU) TINY_ROWS(true, 16, ACT_RELU); else if (act == ACT_LRELU) TINY_ROWS(true, 16, ACT_LRELU); else TINY_ROWS(true, 16, ACT_NONE); }
      else { if (act == ACT_RELU) TINY_ROWS(true, 32, ACT_RELU); else if (act == ACT_LRELU) TINY_ROWS(true, 32, ACT_LRELU); else TINY_ROWS(true, 32, ACT_NONE); }
    } else {
      if (a.N == 16) { if (act == ACT_RELU) TINY_ROWS(false, 16, ACT_RELU); else if (act == ACT_LRELU) TINY_ROWS(false, 16, ACT_LRELU); else TINY_ROWS(false, 16, ACT_NONE); }
      else { if (act == ACT_RELU) TINY_ROWS(false, 32, ACT_RELU); else if (act == ACT_LRELU) TINY_ROWS(false, 32, ACT_LRELU); else TINY_ROWS(false, 32, ACT_NONE); }
    }
#undef TINY_ROWS
    return hipGetLastError();
  }
  long long nb = (total + 255) / 256;
  if (nb > 65536) nb = 65536;
  if (two_d) hipLaunchKernelGGL(conv_tiny_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(conv_tiny_kernel<false>, dim3((unsigned)nb), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace rvcx
