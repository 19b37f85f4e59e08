// Elementwise maps, layout transforms, gathers, masks and the row LayerNorm over time-major [rows][C] matrices, and
// the pipeline's x2 feature upsample + protect blend. HBM- or latency-bound; every kernel keeps channels contiguous
// so a wave reads whole 128-B lines.
#include <algorithm>
#include <cmath>

#include "device_util.h"
#include "rowops_kernels.h"

namespace rvcx {

// ------------------------------------------------------------------ simple maps
__global__ void k_fill(float* p, float v, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    p[i] = v;
}
hipError_t fill(float* p, float v, long long n, hipStream_t s) {
  hipLaunchKernelGGL(k_fill, dim3(nblocks(n)), dim3(TB), 0, s, p, v, n);
  return hipGetLastError();
}

__global__ void k_randn(float* y, long long n, uint64_t seed, uint64_t off) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    y[i] = normal_at(seed, off + i, 0x52564358u, 0u);
}
hipError_t randn(float* y, long long n, uint64_t seed, uint64_t offset, hipStream_t s) {
  hipLaunchKernelGGL(k_randn, dim3(nblocks(n)), dim3(TB), 0, s, y, n, seed, offset);
  return hipGetLastError();
}

__global__ void k_act(float* x, long long n, int act, float slope) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float v = x[i];
    switch (act) {
      case ACT_LRELU: v = v > 0.f ? v : v * slope; break;
      case ACT_RELU: v = v > 0.f ? v : 0.f; break;
      case ACT_GELU: v = 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); break;
      case ACT_TANH: v = tanhf(v); break;
      case ACT_SIGMOID: v = 1.f / (1.f + expf(-v)); break;
      default: break;
    }
    x[i] = v;
  }
}
hipError_t act_inplace(float* x, long long n, int act, float slope, hipStream_t s) {
  hipLaunchKernelGGL(k_act, dim3(nblocks(n)), dim3(TB), 0, s, x, n, act, slope);
  return hipGetLastError();
}

__global__ void k_affine(float* x, long long n, float a, float b) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    x[i] = x[i] * a + b;
}
hipError_t affine_inplace(float* x, long long n, float a, float b, hipStream_t s) {
  hipLaunchKernelGGL(k_affine, dim3(nblocks(n)), dim3(TB), 0, s, x, n, a, b);
  return hipGetLastError();
}

// [B][C][T] -> [B][T][C], 32x32 LDS tiles
__global__ void k_tr(const float* x, float* y, int R, int Cc, long long ld_in, long long ld_out, long long bs_in,
                     long long bs_out) {
  __shared__ float t[32][33];
  const int b = blockIdx.z;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const float* X = x + b * bs_in;
  float* Y = y + b * bs_out;
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + threadIdx.x;
    if (r < R && c < Cc) t[i][threadIdx.x] = X[(long long)r * ld_in + c];
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + threadIdx.x;
    if (r < R && c < Cc) Y[(long long)c * ld_out + r] = t[threadIdx.x][i];
  }
}
hipError_t transpose_bct_btc(const float* x, float* y, int B, int C, int T, hipStream_t s) {
  dim3 g((T + 31) / 32, (C + 31) / 32, B);
  hipLaunchKernelGGL(k_tr, g, dim3(32, 8), 0, s, x, y, C, T, (long long)T, (long long)C, (long long)C * T,
                     (long long)C * T);
  return hipGetLastError();
}

__global__ void k_flip(const float* x, float* y, long long rows, int C) {
  const long long n = rows * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / C;
    const int c = (int)(i - r * C);
    y[i] = x[r * C + (C - 1 - c)];
  }
}
hipError_t channel_flip(const float* x, float* y, int rows, int C, hipStream_t s) {
  hipLaunchKernelGGL(k_flip, dim3(nblocks((long long)rows * C)), dim3(TB), 0, s, x, y, (long long)rows, C);
  return hipGetLastError();
}

__global__ void k_gather(const float* table, int ld, const int32_t* idx, float* y, long long rows, int C) {
  const long long n = rows * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / C;
    const int c = (int)(i - r * C);
    y[i] = table[(long long)idx[r] * ld + c];
  }
}
hipError_t gather_rows(const float* table, int ld_table, const int32_t* idx, float* y, int rows, int C,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_gather, dim3(nblocks((long long)rows * C)), dim3(TB), 0, s, table, ld_table, idx, y,
                     (long long)rows, C);
  return hipGetLastError();
}

__global__ void k_seqmask(const int32_t* len, float* mask, int B, int T) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * T) mask[i] = (i % T) < len[i / T] ? 1.f : 0.f;
}
hipError_t seq_mask(const int32_t* lengths, float* mask, int B, int T, hipStream_t s) {
  hipLaunchKernelGGL(k_seqmask, dim3(nblocks((long long)B * T)), dim3(TB), 0, s, lengths, mask, B, T);
  return hipGetLastError();
}

// ------------------------------------------------------------------ LayerNorm over rows (one wave per row)
__global__ void k_layernorm(const float* x, const float* r, float* y, const float* gamma, const float* beta,
                            int rows, int D, float eps, const float* mask) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= rows) return;
  const float* xr = x + (long long)wave * D;
  const float* rr = r ? r + (long long)wave * D : nullptr;
  float v[16];
  float s = 0.f;
  const int per = (D + 63) / 64;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = lane + j * 64;
    float t = 0.f;
    if (j < per && c < D) {
      t = xr[c];
      if (rr) t = t + rr[c];
    }
    v[j] = t;
    s += t;
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = lane + j * 64;
    if (j < per && c < D) {
      const float d = v[j] - mean;
      q += d * d;
    }
  }
  const float var = wave_sum(q) / (float)D;
  const float rstd = 1.f / sqrtf(var + eps);
  const float mk = mask ? mask[wave] : 1.f;
  float* yr = y + (long long)wave * D;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = lane + j * 64;
    if (j < per && c < D) {
      float o = (v[j] - mean) * rstd * gamma[c] + beta[c];
      if (mask) o *= mk;
      yr[c] = o;
    }
  }
}
hipError_t layernorm_rows(const float* x, const float* r, float* y, const float* gamma, const float* beta,
                          int rows, int D, float eps, const float* mask, hipStream_t s) {
  if (D > 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_layernorm, dim3((rows + 3) / 4), dim3(256), 0, s, x, r, y, gamma, beta, rows, D, eps, mask);
  return hipGetLastError();
}

// ------------------------------------------------------------------ feature x2 upsample + protect blend
// x2 nearest upsample + protect blend (pipeline.py:344-362): feats = retrieved (or raw) features,
// feats0 = raw features; v = feats * p + feats0 * (1 - p) with each product and the sum rounded (torch).
// One launch for all rows (blockIdx.y = row): row b has Lv[b] feature frames -> Tv[b] output frames in out
// [B][T_max][D], frames from Tv[b] on written as zero. feats / feats0 rows of stride L_max frames, pitchf (optional)
// rows of stride ldp.
#pragma clang fp contract(off)
__global__ void k_up2(const float* feats, const float* feats0, Len Lv, int L_max, int D, float* out, Len Tv, int T_max,
                      const float* pitchf, long long ldp, float protect) {
  const int b = blockIdx.y;
  const int L = Lv[b], T = Tv[b];
  feats += (long long)b * L_max * D;
  feats0 += (long long)b * L_max * D;
  out += (long long)b * T_max * D;
  const long long n = (long long)T_max * D;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int t = (int)(i / D), c = (int)(i % D);
    float v = 0.f;
    if (t < T) {
      const int src = t >> 1 < L ? t >> 1 : L - 1;
      const float f = feats[(long long)src * D + c];
      v = f;
      if (pitchf) {
        const float pf = pitchf[b * ldp + t];
        const float p = pf < 1.f ? protect : (pf > 0.f ? 1.f : pf);
        v = f * p + feats0[(long long)src * D + c] * (1.f - p);
      }
    }
    out[i] = v;
  }
}
#pragma clang fp contract(on)
hipError_t upsample2_protect(const float* feats, const float* feats0, Len L, int L_max, int D, float* out, Len T,
                             int T_max, const float* pitchf, long long ldp, float protect, hipStream_t s, int B) {
  if (B < 1 || T_max < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_up2, dim3(std::min(nblocks((long long)T_max * D), 4096u), B), dim3(TB), 0, s, feats, feats0, L,
                     L_max, D, out, T, T_max, pitchf, ldp, protect);
  return hipGetLastError();
}
// pitch [B][ldp] / pitchf [B][ldp] -> pc / pf [B][T_max]: row b's first Tv[b] frames, zero from there on
__global__ void k_pack_pitch(const int32_t* __restrict__ pitch, const float* __restrict__ pitchf, long long ldp,
                             const int* __restrict__ Tv, int T_max, int32_t* __restrict__ pc, float* __restrict__ pf) {
  const int b = blockIdx.y;
  const int T = Tv[b];
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < T_max; t += gridDim.x * blockDim.x) {
    pc[(long long)b * T_max + t] = t < T ? pitch[b * ldp + t] : 0;
    pf[(long long)b * T_max + t] = t < T ? pitchf[b * ldp + t] : 0.f;
  }
}
hipError_t pack_pitch(const int32_t* pitch, const float* pitchf, long long ldp, const int* Tv, int T_max, int32_t* pc,
                      float* pf, int B, hipStream_t s) {
  if (B < 1 || T_max < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pack_pitch, dim3(nblocks(T_max), B), dim3(TB), 0, s, pitch, pitchf, ldp, Tv, T_max, pc, pf);
  return hipGetLastError();
}

}  // namespace rvcx
