// The HiFi-GAN-NSF decoder's non-GEMM kernels: the framed noise conv, the harmonic source (SineGen), conv_post and
// the z_p sampling ahead of the flow. HBM- or latency-bound; time-major rows, channels contiguous.
#include <algorithm>
#include <cmath>

#include "device_util.h"
#include "vocoder_kernels.h"

namespace rvcx {

namespace {
typedef float f32x4v __attribute__((ext_vector_type(4)));
}  // namespace

// ------------------------------------------------------------------ NSF noise conv, accumulated into y
// One thread per 4 consecutive channels of one output row: the row's kk = taps * stride source samples are
// read once for the 4 channels, y is read and written as one float4 (coalesced along the row). The weights are
// staged once per block into LDS as [q][C] so each (q, 4 channels) is one 16-byte read. The per-channel sum runs
// over q in order as an fma chain, then + bias, then + y (the separate-launch order it replaces).
// STORE: y = sum + bias (the noise branch computed ahead into its own buffer, added later as the ConvTranspose's
// residual: y_up + (sum + bias), the same single addition)
constexpr int NOISE_LDS_FLOATS = 4096;
template <bool STORE>
__global__ __launch_bounds__(256) void k_noise_add(const float* __restrict__ har, long long har_bs, int stride,
                                                   int taps, const float* __restrict__ wf,
                                                   const float* __restrict__ nb, float* __restrict__ y, int B, int T,
                                                   int C) {
  __shared__ __attribute__((aligned(16))) float wq[NOISE_LDS_FLOATS];
  const int kk = taps * stride;
  for (int i = threadIdx.x; i < kk * C; i += blockDim.x) {
    const int q = i / C, c = i - q * C;
    const int tap = q / stride, j = q - tap * stride;
    wq[i] = wf[((long long)tap * C + c) * stride + j];
  }
  __syncthreads();
  // 32-bit index arithmetic (the launcher checks B * T * C / 4 < 2^31): 64-bit divisions cost more than the
  // whole per-element body
  const unsigned c4n = (unsigned)C >> 2;
  const unsigned n = (unsigned)B * (unsigned)T * c4n;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const unsigned bt = i / c4n;
    const int c = (int)(i - bt * c4n) << 2;
    const unsigned b = bt / (unsigned)T;
    const long long t = bt - b * (unsigned)T;
    const float* x = har + b * har_bs + t * stride;
    float xs[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) xs[q] = q < kk ? x[q] : 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (q < kk) {
        const float4 w = *reinterpret_cast<const float4*>(wq + q * C + c);
        acc.x = fmaf(w.x, xs[q], acc.x);
        acc.y = fmaf(w.y, xs[q], acc.y);
        acc.z = fmaf(w.z, xs[q], acc.z);
        acc.w = fmaf(w.w, xs[q], acc.w);
      }
    }
    float4* yp = reinterpret_cast<float4*>(y + (long long)bt * C + c);
    if constexpr (STORE) {
      *yp = make_float4(acc.x + nb[c], acc.y + nb[c + 1], acc.z + nb[c + 2], acc.w + nb[c + 3]);
    } else {
      float4 v = *yp;
      v.x = v.x + (acc.x + nb[c]);
      v.y = v.y + (acc.y + nb[c + 1]);
      v.z = v.z + (acc.z + nb[c + 2]);
      v.w = v.w + (acc.w + nb[c + 3]);
      *yp = v;
    }
  }
}
hipError_t noise_conv_add(const float* har, long long har_bs, int stride, int taps, const float* wf, const float* nb,
                          float* y, int B, int T, int C, hipStream_t s, bool store) {
  if (C % 4 != 0 || taps * stride > 16 || taps * stride < 1 || (reinterpret_cast<uintptr_t>(y) & 15) != 0 ||
      (long long)B * T * (C / 4) >= (1LL << 31) || taps * stride * C > NOISE_LDS_FLOATS)
    return hipErrorInvalidValue;
  // grid-stride over a capped grid: each block stages the weights once
  hipLaunchKernelGGL(store ? k_noise_add<true> : k_noise_add<false>,
                     dim3(std::min(nblocks((long long)B * T * (C / 4)), store ? 512u : 4096u)), dim3(TB), 0, s, har,
                     har_bs, stride,
                     taps, wf, nb, y, B, T, C);
  return hipGetLastError();
}

// from here on a product and a sum fuse within one expression only, never across statements
#pragma clang fp contract(on)

// ------------------------------------------------------------------ NSF harmonic source (SineGen, harmonic_num=0)
// SineGen phase prefix (generators/hifigan.py:156-228): rem[l] = fmod(f0[l]/sr*upp + 0.5, 1) - 0.5,
// cum = fmod(cumsum(rem), 1) with the cumsum accumulated in double (torch CPU acc type).
// Parallel scan, bit-identical to torch's sequential double loop: for f0 >= 0, inc + 0.5 >= 0.5 so every
// rem is a multiple of 2^-24 with |rem| <= 0.5, and any partial sum of fewer than 2^28 of them is a
// multiple of 2^-24 below 2^27 in magnitude (51 significant bits): every double addition is exact and the
// summation order cannot change a bit. One block per batch row: each thread sums a contiguous segment, a
// block scan of the segment sums gives each segment's start, and the segment is re-walked to emit
// fmod((float)acc, 1).
constexpr int SINE_T = 1024;
__global__ __launch_bounds__(SINE_T) void k_sine_cum(const float* __restrict__ f0, int B, int L, int upp, float sr,
                                                     double* __restrict__ cum) {
  __shared__ double wsum[SINE_T / 64];
  const int b = blockIdx.x;
  const float* fb = f0 + (long long)b * L;
  float* cf = reinterpret_cast<float*>(cum + (long long)b * L);
  const int n = L - 1;
  if (n <= 0) return;  // block-uniform
  const int per = (n + SINE_T - 1) / SINE_T;
  const int j0 = min(n, (int)threadIdx.x * per), j1 = min(n, j0 + per);
  auto rem_at = [&](int j) {
    const float inc = (fb[j] / sr) * (float)upp;
    return fmodf(inc + 0.5f, 1.0f) - 0.5f;
  };
  double s = 0.0;
  for (int j = j0; j < j1; ++j) s += (double)rem_at(j);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double v = s;  // inclusive scan over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  if (lane == 63) wsum[w] = v;
  __syncthreads();
  double acc = v - s;
  for (int k = 0; k < w; ++k) acc += wsum[k];
  for (int j = j0; j < j1; ++j) {
    acc += (double)rem_at(j);
    cf[j] = fmodf((float)acc, 1.0f);
  }
}
__global__ void k_sine(const float* f0, int B, int L, int upp, float sr, const double* cum, const float* eps,
                       uint64_t seed, float lin_w, float lin_b, float* har, long long har_ld) {
  const long long n = (long long)B * L * upp;
  const float two_pi = 6.283185307179586f;
  const float amp_unv = (float)(0.1 / 3.0);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int u = (int)(i % upp);
    const long long bl = i / upp;
    const int b = (int)(bl / L), l = (int)(bl % L);
    const float f = f0[bl];
    float ph = (f / sr) * (float)(u + 1);
    if (l > 0) ph = ph + reinterpret_cast<const float*>(cum + (long long)b * L)[l - 1];
    const float sine = sinf(two_pi * ph) * 0.1f;
    const float uv = f > 0.f ? 1.f : 0.f;
    const float amp = uv * 0.003f + (1.f - uv) * amp_unv;
    const float e = eps ? eps[i] : normal_at(seed, (uint64_t)i, 0x52564358u, 0u);
    const float merged = sine * uv + amp * e;
    har[(long long)b * har_ld + (long long)l * upp + u] = tanhf(merged * lin_w + lin_b);
  }
}
hipError_t sine_source(const float* f0, int B, int L, int upp, float sr, const float* eps, uint64_t seed,
                       float lin_w, float lin_b, double* cum_ws, float* har, long long har_ld, hipStream_t s) {
  hipLaunchKernelGGL(k_sine_cum, dim3(B), dim3(SINE_T), 0, s, f0, B, L, upp, sr, cum_ws);
  hipLaunchKernelGGL(k_sine, dim3(nblocks((long long)B * L * upp)), dim3(TB), 0, s, f0, B, L, upp, sr, cum_ws, eps,
                     seed, lin_w, lin_b, har, har_ld);
  return hipGetLastError();
}

// ------------------------------------------------------------------ conv_post: tanh(conv1d(lrelu(x, 0.01), w[1][C][K], pad K/2)), no bias
// The C*K weights sit in LDS too: read from global inside the FMA loop (uniform address, possibly
// aliasing y) they were one dependent vector load per FMA (80 us at C2).
// LeakyReLU -> Conv1d(C -> 1, K taps) -> tanh over 256 output samples per block. The lrelu'd input tile (+ halo)
// is staged in LDS with an odd row stride (conflict-free column reads); it is fetched as float4 loads all issued
// before the first LDS store (CP_IT per thread), so a block waits for one load latency, not one per element.
constexpr int CP_T = 256, CP_IT = 24;  // C <= 92 at K = 7
__global__ __launch_bounds__(CP_T) void k_conv_post(const float* __restrict__ x, int T, int C,
                                                    const float* __restrict__ wg, int K, float slope,
                                                    float* __restrict__ y, float bias, long long y_bs) {
  extern __shared__ float tile[];  // [(CP_T+K-1)][C+1], then w[C*K]
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * CP_T;
  const int pad = K / 2;
  const int rows = CP_T + K - 1;
  const int ldt = C + 1;
  const int C4 = C >> 2;
  float* w = tile + rows * ldt;
  for (int i = threadIdx.x; i < C * K; i += blockDim.x) w[i] = wg[i];
  const float* xb = x + (long long)b * T * C;
  f32x4v v[CP_IT];
#pragma unroll
  for (int it = 0; it < CP_IT; ++it) {
    const int idx = it * CP_T + threadIdx.x;
    const int r = idx / C4, c4 = (idx - r * C4) * 4;
    const int g = t0 - pad + r;
    v[it] = (r < rows && g >= 0 && g < T) ? *reinterpret_cast<const f32x4v*>(xb + (long long)g * C + c4)
                                          : f32x4v{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int it = 0; it < CP_IT; ++it) {
    const int idx = it * CP_T + threadIdx.x;
    const int r = idx / C4, c4 = (idx - r * C4) * 4;
    if (r < rows) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float u = v[it][e];
        tile[r * ldt + c4 + e] = u > 0.f ? u : u * slope;
      }
    }
  }
  __syncthreads();
  const int t = t0 + threadIdx.x;
  if (t >= T) return;
  float acc = 0.f;
  for (int c = 0; c < C; ++c)
    for (int k = 0; k < K; ++k) acc = fmaf(tile[(threadIdx.x + k) * ldt + c], w[c * K + k], acc);
  y[(long long)b * y_bs + t] = tanhf(acc + bias);  // + 0 for the bias-free HiFi-GAN / RefineGAN conv_post
}
// The same conv_post at the HiFi-GAN-NSF / MRF shape (C = 32, K = 7: every RVC v2 rate): C and K at compile time,
// the lrelu'd tile in LDS with a 36-float row stride (16 consecutive rows' float4 reads hit 64 distinct banks), the
// weights as one float4 per (tap, 4 channels) broadcast, and the 224 products of an output in four independent fma
// chains per float4 lane (the generic kernel's single dependent chain of 224 LDS-fed fmas ran at 73 us for 744000
// samples, ~1/5 of the HBM rate for its 95 MB). Summation order: channel group c4 outer, tap inner per chain, the
// four chains added at the end: the result differs from the generic kernel's in the last bits only.
constexpr int CPF_C = 32, CPF_K = 7, CPF_LD = 36, CPF_ROWS = CP_T + CPF_K - 1;
__global__ __launch_bounds__(CP_T) void k_conv_post32(const float* __restrict__ x, int T,
                                                      const float* __restrict__ wg, float slope,
                                                      float* __restrict__ y, float bias, long long y_bs) {
  __shared__ __attribute__((aligned(16))) float tile[CPF_ROWS * CPF_LD];
  __shared__ __attribute__((aligned(16))) float w[CPF_K * CPF_C];  // [k][c]
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * CP_T;
  constexpr int pad = CPF_K / 2;
  constexpr int C4 = CPF_C / 4;
  constexpr int IT = (CPF_ROWS * C4 + CP_T - 1) / CP_T;
  if (threadIdx.x < CPF_K * CPF_C) {
    const int k = threadIdx.x / CPF_C, c = threadIdx.x - k * CPF_C;
    w[threadIdx.x] = wg[c * CPF_K + k];
  }
  const float* xb = x + (long long)b * T * CPF_C;
  f32x4v v[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int idx = it * CP_T + threadIdx.x;
    const int r = idx / C4, c4 = (idx - r * C4) * 4;
    const int g = t0 - pad + r;
    const bool ok = r < CPF_ROWS && g >= 0 && g < T;
    v[it] = *reinterpret_cast<const f32x4v*>(xb + (long long)(ok ? g : 0) * CPF_C + c4);
    if (!ok) v[it] = f32x4v{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int idx = it * CP_T + threadIdx.x;
    const int r = idx / C4, c4 = (idx - r * C4) * 4;
    if (r < CPF_ROWS) {
      f32x4v u = v[it];
#pragma unroll
      for (int e = 0; e < 4; ++e) u[e] = u[e] > 0.f ? u[e] : u[e] * slope;
      *reinterpret_cast<f32x4v*>(&tile[r * CPF_LD + c4]) = u;
    }
  }
  __syncthreads();
  const int t = t0 + threadIdx.x;
  if (t >= T) return;
  f32x4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c4 = 0; c4 < C4; ++c4)
#pragma unroll
    for (int k = 0; k < CPF_K; ++k) {
      const f32x4v xv = *reinterpret_cast<const f32x4v*>(&tile[(threadIdx.x + k) * CPF_LD + 4 * c4]);
      const f32x4v wv = *reinterpret_cast<const f32x4v*>(&w[k * CPF_C + 4 * c4]);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(xv[e], wv[e], acc[e]);
    }
  y[(long long)b * y_bs + t] = tanhf(((acc[0] + acc[1]) + (acc[2] + acc[3])) + bias);
}

hipError_t conv_post_tanh(const float* x, int B, int T, int C, const float* w, int K, float slope, float* y,
                          hipStream_t s, float bias, long long y_bs) {
  if (y_bs <= 0) y_bs = T;
  if (C == CPF_C && K == CPF_K && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    hipLaunchKernelGGL(k_conv_post32, dim3((T + CP_T - 1) / CP_T, B), dim3(CP_T), 0, s, x, T, w, slope, y, bias,
                       y_bs);
    return hipGetLastError();
  }
  // the staged fetch covers (CP_T + K - 1) rows of C / 4 float4 in CP_IT rounds of CP_T threads
  if (C % 4 != 0 || (long long)(CP_T + K - 1) * (C / 4) > (long long)CP_IT * CP_T ||
      (reinterpret_cast<uintptr_t>(x) & 15) != 0)
    return hipErrorInvalidValue;
  const size_t smem = ((size_t)(CP_T + K - 1) * (C + 1) + (size_t)C * K) * sizeof(float);
  hipLaunchKernelGGL(k_conv_post, dim3((T + CP_T - 1) / CP_T, B), dim3(CP_T), smem, s, x, T, C, w, K, slope, y, bias,
                     y_bs);
  return hipGetLastError();
}

// ------------------------------------------------------------------ z_p = (m + exp(logs) * eps * 0.66666) * mask
// stats: [B][T][2I] (m | logs); eps (reference layout [B][I][T]) or generated.
__global__ void k_zp(const float* stats, int B, int T, int I, const float* eps, uint64_t seed, const float* mask,
                     float* zp) {
  const long long n = (long long)B * T * I;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % I);
    const long long bt = i / I;
    const int b = (int)(bt / T), t = (int)(bt % T);
    const float m = stats[bt * 2 * I + c];
    const float lg = stats[bt * 2 * I + I + c];
    const long long ei = ((long long)b * I + c) * T + t;
    const float e = eps ? eps[ei] : normal_at(seed, (uint64_t)ei, 0x52564358u, 0u);
    zp[i] = (m + expf(lg) * e * 0.66666f) * mask[bt];
  }
}
hipError_t zp_sample(const float* stats, int B, int T, int I, const float* eps, uint64_t seed, const float* mask,
                     float* zp, hipStream_t s) {
  hipLaunchKernelGGL(k_zp, dim3(nblocks((long long)B * T * I)), dim3(TB), 0, s, stats, B, T, I, eps, seed, mask, zp);
  return hipGetLastError();
}

}  // namespace rvcx
