// RMVPE's non-GEMM kernels: the reflect pads and STFT magnitude of its mel front end (the magnitude is FCPE's too),
// the U-Net's pooling, layout change and up-conv weight packing, and the salience decode.
#include <algorithm>
#include <cmath>

#include "device_util.h"
#include "fe_kernels.h"

namespace rvcx {

// ------------------------------------------------------------------ ConvTranspose2d 3x3 s2 p1 op1 as a 2x2-tap phase conv
// w [C][co][3][3] (torch layout) -> [tap = 2 dh + dw][4 co][C]: virtual column (ph 2 + pw) co + o of input offset (dh,
// dw) takes kernel tap (kmap[ph][dh], kmap[pw][dw]) with kmap = {{1, -1}, {2, 0}} (-1: no tap, zero); the runtime's
// packing of the U-Net decoder's up-conv (runtime_fe.cpp, BN scale 1)
__global__ void k_upconv_pack(const float* __restrict__ w, int C, int co, float* __restrict__ out) {
  const long long total = 4LL * 4 * co * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ii = (int)(i % C);
    const long long r = i / C;
    const int n = (int)(r % (4 * co)), tap = (int)(r / (4 * co));
    const int dh = tap >> 1, dw = tap & 1, ph = n / (2 * co), pw = (n / co) & 1, o = n % co;
    const int kmap[2][2] = {{1, -1}, {2, 0}};
    const int kh = kmap[ph][dh], kw = kmap[pw][dw];
    out[i] = (kh < 0 || kw < 0) ? 0.f : w[(((long long)ii * co + o) * 3 + kh) * 3 + kw];
  }
}

hipError_t upconv_phase_pack(const float* w, int C, int co, float* out, hipStream_t s) {
  const long long total = 16LL * co * C;
  hipLaunchKernelGGL(k_upconv_pack, dim3((unsigned)std::min<long long>((total + 255) / 256, 8192)), dim3(256), 0, s,
                     w, C, co, out);
  return hipGetLastError();
}

// from here on a product and a sum fuse within one expression only, never across statements
#pragma clang fp contract(on)

// ------------------------------------------------------------------ RMVPE front end
// grid.y = sequence: x rows of stride ldx, y rows of stride ldy; sequence b has n[b] samples and is reflected about
// its own ends (samples past n[b] are never read)
// (a row stride ldy past the padded length gets its tail zeroed here: no fill launch before)
__global__ void k_reflect1d(const float* x, Len nv, int pl, int pr, float* y, long long ldx, long long ldy) {
  const int n = nv[blockIdx.y];
  const int m = n + pl + pr;
  const int mz = ldy > m ? (int)ldy : m;
  x += blockIdx.y * ldx;
  y += blockIdx.y * ldy;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < mz; i += gridDim.x * blockDim.x) {
    int j = i - pl;
    if (j < 0) j = -j;
    if (j >= n) j = 2 * (n - 1) - j;
    y[i] = i < m ? x[j] : 0.f;
  }
}
hipError_t reflect_pad_1d(const float* x, int n, int pad_l, int pad_r, float* y, hipStream_t s, int B, long long ldx,
                          long long ldy, const int* nv) {
  if (pad_l >= n || pad_r >= n || (nv && ldy < (long long)n + pad_l + pad_r)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_reflect1d, dim3(std::min(nblocks(n + pad_l + pad_r), 2048u), B), dim3(TB), 0, s, x,
                     nv ? Len(nv) : Len(n), pad_l, pad_r, y, ldx, ldy);
  return hipGetLastError();
}
// grid.y = image: x [B][ld_in][C] -> y [B][ld_out][C]; image b's rows[b] rows, then their reflection up to out[b]
// rows, then zeros up to ld_out
__global__ void k_reflect_rows(const float* x, Len rowsv, Len outv, int ld_in, int ld_out, int C, float* y) {
  const int rows = rowsv[blockIdx.y], out = outv[blockIdx.y];
  const long long n = (long long)ld_out * C;
  x += (long long)blockIdx.y * ld_in * C;
  y += (long long)blockIdx.y * n;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / C), c = (int)(i % C);
    const int src = r < rows ? r : 2 * (rows - 1) - r;
    y[i] = r < out ? x[(long long)src * C + c] : 0.f;
  }
}
hipError_t reflect_pad_rows(const float* x, int rows, int C, int pad_r, float* y, hipStream_t s, int B) {
  if (pad_r >= rows) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_reflect_rows, dim3(std::min(nblocks((long long)(rows + pad_r) * C), 2048u), B), dim3(TB), 0,
                     s, x, Len(rows), Len(rows + pad_r), rows, rows + pad_r, C, y);
  return hipGetLastError();
}
// images of different heights: rows[b] (device) of ld_in, padded to out[b] (device, out[b] - rows[b] < rows[b]: the
// caller's check) of ld_out
hipError_t reflect_pad_rows_v(const float* x, const int* rows, const int* out, int ld_in, int ld_out, int C, float* y,
                              hipStream_t s, int B) {
  hipLaunchKernelGGL(k_reflect_rows, dim3(std::min(nblocks((long long)ld_out * C), 2048u), B), dim3(TB), 0, s, x,
                     Len(rows), Len(out), ld_in, ld_out, C, y);
  return hipGetLastError();
}
// sqrt(re^2 + im^2 + eps) in rows of ldm floats: bins 0 .. nb - 1, then zeros up to ldm (the mel GEMM's contraction
// runs over whole 32-bin chunks). eps is 0 (RMVPE) or 1e-9 (FCPE.py:154), one instantiation each, so that each caller
// keeps the arithmetic its own kernel had: RMVPE's sum contracted to one FMA, FCPE's with every product and sum rounded
template <bool EPS>
__global__ void k_stftmag(const float* spec, int F, int nb, float* mag, int ldm) {
  const long long n = (long long)F * ldm;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int f = (int)(i / ldm), k = (int)(i % ldm);
    float v = 0.f;
    if (k < nb) {
      const float re = spec[(long long)f * 2 * nb + k];
      const float im = spec[(long long)f * 2 * nb + nb + k];
      v = EPS ? sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)), 1e-9f)) : sqrtf(re * re + im * im);
    }
    mag[i] = v;
  }
}
hipError_t stft_magnitude(const float* spec, int F, int nbins, float eps, float* mag, int ldm, hipStream_t s) {
  if (ldm < nbins || (eps != 0.f && eps != 1e-9f)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(eps != 0.f ? k_stftmag<true> : k_stftmag<false>, dim3(nblocks((long long)F * ldm)), dim3(TB), 0, s,
                     spec, F, nbins, mag, ldm);
  return hipGetLastError();
}

__global__ void k_avgpool2(const float* x, int H, int W, int C, int ldx, float* y) {
  const int Ho = H / 2, Wo = W / 2;
  const long long n = (long long)Ho * Wo * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long long p = i / C;
    const int h = (int)(p / Wo), w = (int)(p % Wo);
    const float* a = x + ((long long)(2 * h) * W + 2 * w) * ldx + c;
    const float* bb = a + (long long)W * ldx;
    y[i] = (((a[0] + a[ldx]) + bb[0]) + bb[ldx]) / 4.f;
  }
}
hipError_t avgpool2(const float* x, int H, int W, int C, int ldx, float* y, hipStream_t s) {
  hipLaunchKernelGGL(k_avgpool2, dim3(nblocks((long long)(H / 2) * (W / 2) * C)), dim3(TB), 0, s, x, H, W, C, ldx, y);
  return hipGetLastError();
}

__global__ void k_nhwc_hcw(const float* x, int H, int W, int C, float* y) {
  const long long n = (long long)H * W * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int h = (int)(i / (W * C));
    const int rem = (int)(i % (W * C));
    const int c = rem / W, w = rem % W;
    y[i] = x[((long long)h * W + w) * C + c];
  }
}
hipError_t nhwc_to_hcw(const float* x, int H, int W, int C, float* y, hipStream_t s) {
  hipLaunchKernelGGL(k_nhwc_hcw, dim3(nblocks((long long)H * W * C)), dim3(TB), 0, s, x, H, W, C, y);
  return hipGetLastError();
}

// ------------------------------------------------------------------ RMVPE decode (RMVPE.py:484-540), fp64 like numpy
// rows of B sequences: frame f < F[b] of sequence b reads sal[(b*Fs + f)][.] and writes f0[b*ldf + f]
__global__ void k_decode(const float* sal, Len Fv, int F, int Fs, int nrows, int ncls, float thred, double* f0,
                         long long ldf) {
#pragma clang fp contract(off)  // numpy rounds every product and sum separately
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= nrows) return;
  const int b = row / F, f = row % F;
  if (f >= Fv[b]) return;
  const float* s = sal + ((long long)b * Fs + f) * ncls;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int k = lane; k < ncls; k += 64) {
    const float v = s[k];
    if (v > best) {
      best = v;
      bi = k;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    // numpy reduces each 9-wide row with its pairwise kernel: 8 partials seeded by a[0..7], combined
    // ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then + a[8]. weight_sum stays float32 (salience dtype),
    // product_sum is float64 (float32 * float64 cents map). Out-of-range slots are the zero padding.
    float wv[9];
    double pv[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int k = bi - 4 + j;
      const bool in = k >= 0 && k < ncls;
      wv[j] = in ? s[k] : 0.f;
      pv[j] = in ? (double)wv[j] * (20.0 * k + 1997.3794084376191) : 0.0;
    }
    const float wsf = (((wv[0] + wv[1]) + (wv[2] + wv[3])) + ((wv[4] + wv[5]) + (wv[6] + wv[7]))) + wv[8];
    const double ps = (((pv[0] + pv[1]) + (pv[2] + pv[3])) + ((pv[4] + pv[5]) + (pv[6] + pv[7]))) + pv[8];
    const double ws = (double)wsf;
    double cents = ps / ws;
    if ((double)best <= (double)thred) cents = 0.0;
    double v = 10.0 * pow(2.0, cents / 1200.0);
    if (v == 10.0) v = 0.0;
    f0[b * ldf + f] = v;
  }
}
hipError_t rmvpe_decode(const float* sal, int F, int ncls, float thred, double* f0, hipStream_t s, int B, int Fs,
                        const int* Fv, long long ldf) {
  if (Fs <= 0) Fs = F;
  if (ldf <= 0) ldf = F;
  const int nrows = B * F;
  hipLaunchKernelGGL(k_decode, dim3((nrows + 3) / 4), dim3(256), 0, s, sal, Fv ? Len(Fv) : Len(F), F, Fs, nrows, ncls,
                     thred, f0, ldf);
  return hipGetLastError();
}

}  // namespace rvcx
