// The split-K combine kernels: the ksplit partial tiles of a split launch (every conv family writes the same slab) summed
// in slice order, then the epilogue -- the shared one, the post-norm LayerNorm's, or the WaveNet gate's.
#include <algorithm>

#include "conv_common.h"
#include "device_util.h"

namespace rvcx {

// split-K combine: sums the ksplit partial tiles in slice order (deterministic) and applies the epilogue. Grid
// (x: elements of one batch entry, y: batch entry); 32-bit element index within an entry (launch checks), all
// ksplit slab loads of an element issued before the ordered sum
__global__ void splitk_reduce_kernel(const ConvArgs a, const int ksplit, const int two_d) {
  const unsigned per_b = (unsigned)(a.ws_rows * a.N);
  const int zb = blockIdx.y;
  const int b = zb / a.batch_inner, bi = zb - (zb / a.batch_inner) * a.batch_inner;
  const EpiPtrs e = epi_ptrs(a, b, bi);
  const float* base = a.ws + (long long)zb * ksplit * per_b;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < per_b; i += gridDim.x * blockDim.x) {
    const unsigned m = i / (unsigned)a.N;
    const int n = (int)(i - m * (unsigned)a.N);
    const float* p = base + i;
    float v = 0.f;
    int s = 0;
    for (; s + 4 <= ksplit; s += 4) {
      const float p0 = p[(long long)s * per_b], p1 = p[(long long)(s + 1) * per_b];
      const float p2 = p[(long long)(s + 2) * per_b], p3 = p[(long long)(s + 3) * per_b];
      v += p0;
      v += p1;
      v += p2;
      v += p3;
    }
    for (; s < ksplit; ++s) v += p[(long long)s * per_b];
    int oh = 0, ow = 0;
    if (two_d) {
      oh = (int)(m / (unsigned)a.W_out);
      ow = (int)(m - (unsigned)oh * (unsigned)a.W_out);
    }
    epilogue_store(a, v, e.bias ? e.bias[n] : 0.f, m, n, oh, ow, e);
  }
}

// split-K combine + the post-norm LayerNorm (ConvArgs::ln_g): one 256-thread block per output row, thread t holding
// columns t + 256 j (N <= 1024); every slab load of a column issued before its ordered sum, as in splitk_reduce_kernel
// (a wave per row with the loads in a column loop measured 16 us against 5.6 + 7 for the two passes). The arithmetic
// is splitk_reduce_kernel's epilogue followed by k_layernorm's on (res + v); the mean and variance sum the columns in
// another order (block-wide), so the result equals the two passes to fp32 rounding of those sums.
__global__ __launch_bounds__(256) void splitk_reduce_ln_kernel(const ConvArgs a, const int ksplit) {
  __shared__ float red[2][4];
  const long long row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = (int)(row / a.ws_rows);
  const long long m = row - (long long)b * a.ws_rows;
  const long long per_b = a.ws_rows * a.N;
  const EpiPtrs e = epi_ptrs(a, b, 0);
  const float* R = e.R + m * a.ldr;  // the LayerNorm's residual input (the launch checks it is there)
  const float mk = e.MK ? e.MK[m] : 1.f;
  float* Y = e.Y + m * a.ldy;
  const float* base = a.ws + (long long)b * ksplit * per_b + m * a.N;
  float v[4];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = tid + j * 256;
    float t = 0.f;
    if (n < a.N) {
      const float* p = base + n;
      float acc = 0.f;
      int k = 0;
      for (; k + 4 <= ksplit; k += 4) {  // splitk_reduce_kernel's order
        const float p0 = p[(long long)k * per_b], p1 = p[(long long)(k + 1) * per_b];
        const float p2 = p[(long long)(k + 2) * per_b], p3 = p[(long long)(k + 3) * per_b];
        acc += p0;
        acc += p1;
        acc += p2;
        acc += p3;
      }
      for (; k < ksplit; ++k) acc += p[(long long)k * per_b];
      // the epilogue's bias, alpha, activation, mask (the launch checks RES_NONE and ACC_STORE)
      float v1[1] = {acc};
      epi_math<1>(a, v1, e.bias ? e.bias[n] : 0.f, 0.f, 0.f);
      epi_mask<1>(e.MK, v1, mk);
      t = R[n];
      t = t + v1[0];
    }
    v[j] = t;
    s += t;
  }
  s = wave_sum(s);
  if (lane == 0) red[0][wave] = s;
  __syncthreads();
  const float mean = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)a.N;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = tid + j * 256;
    if (n < a.N) {
      const float d = v[j] - mean;
      q += d * d;
    }
  }
  q = wave_sum(q);
  if (lane == 0) red[1][wave] = q;
  __syncthreads();
  const float var = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)a.N;
  const float rstd = 1.f / sqrtf(var + a.ln_eps);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = tid + j * 256;
    if (n < a.N) Y[n] = (v[j] - mean) * rstd * a.ln_g[n] + a.ln_b[n];
  }
}

namespace {

// the split-K combine of a gated WaveNet in_layer (ConvArgs::gate_h): the pair (c, c + H) of one output row per thread
// (tanh(u) * sigmoid(v), each with the conditioning added first), acts [rows][ldy]
__global__ void splitk_reduce_gate_kernel(const ConvArgs a, const int ksplit) {
  const unsigned H = (unsigned)a.gate_h;
  const unsigned per_b = (unsigned)(a.ws_rows * a.N), per_o = (unsigned)a.ws_rows * H;
  const int b = blockIdx.y;
  const float* g = a.gate_g + (long long)b * a.gate_g_bs;
  float* Y = a.y + (long long)b * a.y_bs;
  const float* base = a.ws + (long long)b * ksplit * per_b;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < per_o; i += gridDim.x * blockDim.x) {
    const unsigned m = i / H, c = i - m * H;
    const float* p = base + (size_t)m * a.N + c;
    float u = 0.f, v = 0.f;
    for (int s = 0; s < ksplit; ++s) {
      u += p[(long long)s * per_b];
      v += p[(long long)s * per_b + H];
    }
    if (a.bias) {
      u += a.bias[c];
      v += a.bias[c + H];
    }
    const float ta = u + g[c], sb = v + g[c + H];
    Y[(long long)m * a.ldy + c] = tanhf(ta) * (1.f / (1.f + expf(-sb)));
  }
}

}  // namespace

hipError_t launch_splitk_reduce(const ConvArgs& a, int ksplit, bool two_d, hipStream_t s) {
  if (a.ln_g) {
    if (two_d || a.batch_inner != 1 || a.N > 1024 || !a.ln_b || !a.res || a.res_mode != RES_NONE ||
        a.acc_mode != ACC_STORE || a.out_map != OUT_ROWS || a.gate_h > 0)
      return hipErrorInvalidValue;
    const long long rows = (long long)a.batch * a.ws_rows;
    if (rows >= (1LL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(splitk_reduce_ln_kernel, dim3((unsigned)rows), dim3(256), 0, s, a, ksplit);
    return hipGetLastError();
  }
  if (a.gate_h > 0) {
    if (two_d || a.batch_inner != 1 || a.N != 2 * a.gate_h || !a.gate_g) return hipErrorInvalidValue;
    const long long per_o = a.ws_rows * a.gate_h;
    hipLaunchKernelGGL(splitk_reduce_gate_kernel, dim3((unsigned)std::min<long long>((per_o + 255) / 256, 4096),
                                                       (unsigned)a.batch), dim3(256), 0, s, a, ksplit);
    return hipGetLastError();
  }
  const long long per_b = (long long)a.ws_rows * a.N;
  const int nz = a.batch * a.batch_inner;
  if (per_b >= (1LL << 31) || nz > 65535) return hipErrorInvalidValue;  // 32-bit element index, grid y
  long long nb = (per_b + 255) / 256;
  if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)nb, (unsigned)nz), dim3(256), 0, s, a, ksplit,
                     two_d ? 1 : 0);
  return hipGetLastError();
}

}  // namespace rvcx
