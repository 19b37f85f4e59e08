// The realtime noise gate: noisereduce.torchgate.TorchGate's stationary mode as rvc/realtime/core.py:86-94 builds it
// (TorchGate(tgt_sr, prop_decrease=clean_strength), no separate noise clip) and rvc/realtime/pipeline.py:326-327
// applies it to a hop's model output. Over x [B][n]:
//   X     = stft(x, 1024, hop 256, periodic Hann, center=True with ZERO padding)           [B][F][513], F = 1 + n / 256
//   X_db  = 20 log10(|X| + eps), clamped per (row, bin) to its maximum over frames - 40
//   mask  = X_db > mean_t(X_db) + 1.5 std_t(X_db)   (unbiased std)
//   s     = conv2d(mask ? 1 : 1 - p, outer(v_f, v_t) / sum, zeros outside)   (triangles of 500 Hz and 50 ms half width)
//   y     = istft(X s)   [B][256 (F - 1)]: windowed overlap-add / overlap-added squared window, 512 samples trimmed
// Four launches whatever B is: k_sg_forward (one frame per block), k_sg_stats (64 bins of one row per block),
// k_sg_back (one frame per block: smoothing, product, inverse FFT, window), k_sg_ola (one output sample per thread: its
// up to four frames gathered in ascending frame order, so the sum is the same from run to run; no atomics).
// Rows whose strength is negative are not gated: the first three kernels leave at once and k_sg_ola copies x through.
//
// The FFT: 1024 complex points in LDS, radix-4 Stockham (five passes, 256 threads, one butterfly each), fp32 with the
// twiddles exp(-2 pi i m / 1024) from a table made in double on the host. Real and imaginary parts lie in separate
// planes: a pass reads src[j + 256 r] (unit stride over the lanes, no bank conflict) and writes dst[(j / Ns) 4 Ns +
// j % Ns + r Ns]; that write has a lane stride of 4 words in the first pass (4 lanes per bank of the 64) and is
// conflict-free from the third pass on. Five passes of 4 KiB are far below what one launch costs here, so the planes
// are not padded.
#include <hip/hip_runtime.h>

#include <cmath>

#include "stream_kernels.h"

namespace rvcx {

namespace {
constexpr int SG_N = SG_NFFT, SG_TB = 256;
constexpr float SG_EPS = 2.220446049250313e-16f;  // torch.finfo(float64).eps, as TorchGate adds it in any dtype

// a[0..1023] -> the transform in b (five passes ping-pong a -> b -> a -> b -> a -> b). INV: conjugate twiddles, no 1/N.
template <bool INV>
__device__ __forceinline__ void fft1024(float* ar, float* ai, float* br, float* bi, const float2* __restrict__ tw) {
  const int j = threadIdx.x;
  float *sr = ar, *si = ai, *dr = br, *di = bi;
#pragma unroll
  for (int Ns = 1; Ns < SG_N; Ns <<= 2) {
    const int k = j & (Ns - 1);
    const int step = (SG_N / 4) / Ns;
    float vr[4], vi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      vr[r] = sr[j + 256 * r];
      vi[r] = si[j + 256 * r];
    }
#pragma unroll
    for (int r = 1; r < 4; ++r) {
      const float2 w = tw[r * k * step];  // r k step < 768
      const float wr = w.x, wi = INV ? -w.y : w.y;
      const float a = vr[r], b = vi[r];
      vr[r] = a * wr - b * wi;
      vi[r] = a * wi + b * wr;
    }
    const float t0r = vr[0] + vr[2], t0i = vi[0] + vi[2];
    const float t1r = vr[0] - vr[2], t1i = vi[0] - vi[2];
    const float t2r = vr[1] + vr[3], t2i = vi[1] + vi[3];
    // (v1 - v3) times -i (forward) or +i (inverse)
    const float dr3 = vr[1] - vr[3], di3 = vi[1] - vi[3];
    const float t3r = INV ? -di3 : di3, t3i = INV ? dr3 : -dr3;
    const int j0 = ((j - k) << 2) + k;
    dr[j0] = t0r + t2r;
    di[j0] = t0i + t2i;
    dr[j0 + Ns] = t1r + t3r;
    di[j0 + Ns] = t1i + t3i;
    dr[j0 + 2 * Ns] = t0r - t2r;
    di[j0 + 2 * Ns] = t0i - t2i;
    dr[j0 + 3 * Ns] = t1r - t3r;
    di[j0 + 3 * Ns] = t1i - t3i;
    __syncthreads();
    float* t = sr;
    sr = dr;
    dr = t;
    t = si;
    si = di;
    di = t;
  }
}

// one frame of one row: zero-padded framing, window, FFT; X [B][F][513] (re, im) and X_db [B][F][513]
__global__ void __launch_bounds__(SG_TB) k_sg_forward(const float* __restrict__ x, long long ldx, long long n, int F,
                                                      const float* __restrict__ strength,
                                                      const float* __restrict__ tab, float2* __restrict__ X,
                                                      float* __restrict__ db) {
  __shared__ float ar[SG_N], ai[SG_N], br[SG_N], bi[SG_N];
  const int b = blockIdx.y, t = blockIdx.x;
  if (strength[b] < 0.f) return;
  const float2* tw = reinterpret_cast<const float2*>(tab);
  const float* win = tab + 2 * SG_N;
  const float* xb = x + b * ldx;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = threadIdx.x + 256 * r;
    const long long src = (long long)t * SG_HOP - SG_N / 2 + i;
    ar[i] = (src >= 0 && src < n) ? xb[src] * win[i] : 0.f;
    ai[i] = 0.f;
  }
  __syncthreads();
  fft1024<false>(ar, ai, br, bi, tw);
  const long long o = ((long long)b * F + t) * SG_BINS;
  for (int f = threadIdx.x; f < SG_BINS; f += SG_TB) {
    const float re = br[f], im = bi[f];
    X[o + f] = make_float2(re, im);
    db[o + f] = 20.f * log10f(sqrtf(re * re + im * im) + SG_EPS);
  }
}

// 64 bins of one row: the maximum over frames, the clamp, mean and unbiased std in fp64, the threshold, the mask.
// Thread (g, lane) takes bin blockIdx.x * 64 + lane and the frames g, g + 4, ...; the four partial results of a bin
// are combined in the order g = 0..3.
__global__ void __launch_bounds__(SG_TB) k_sg_stats(const float* __restrict__ db, int F,
                                                    const float* __restrict__ strength,
                                                    unsigned char* __restrict__ mask,
                                                    unsigned char* __restrict__ mask_out) {
  __shared__ double red[4][64];
  const int b = blockIdx.y;
  if (strength[b] < 0.f) return;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int f = blockIdx.x * 64 + lane;
  const bool live = f < SG_BINS;
  const float* d = db + (long long)b * F * SG_BINS + (live ? f : 0);
  float m = -INFINITY;
  if (live)
    for (int t = g; t < F; t += 4) m = fmaxf(m, d[(long long)t * SG_BINS]);
  red[g][lane] = (double)m;
  __syncthreads();
  const float mx = (float)fmax(fmax(red[0][lane], red[1][lane]), fmax(red[2][lane], red[3][lane]));
  const float floor_db = mx - 40.f;
  __syncthreads();
  double acc = 0.0;
  if (live)
    for (int t = g; t < F; t += 4) acc += (double)fmaxf(d[(long long)t * SG_BINS], floor_db);
  red[g][lane] = acc;
  __syncthreads();
  const double mean = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) / (double)F;
  __syncthreads();
  acc = 0.0;
  if (live)
    for (int t = g; t < F; t += 4) {
      const double e = (double)fmaxf(d[(long long)t * SG_BINS], floor_db) - mean;
      acc += e * e;
    }
  red[g][lane] = acc;
  __syncthreads();
  const double var = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) / (double)(F - 1);
  const double thr = mean + 1.5 * sqrt(var);
  if (!live) return;
  unsigned char* mk = mask + (long long)b * F * SG_BINS + f;
  for (int t = g; t < F; t += 4) {
    const unsigned char v = (double)fmaxf(d[(long long)t * SG_BINS], floor_db) > thr ? 1 : 0;
    mk[(long long)t * SG_BINS] = v;
    if (mask_out) mask_out[((long long)b * SG_BINS + f) * F + t] = v;
  }
}

// triangle tap d in [-m, m] of the normalised filter: ((m + 1 - |d|) / (m + 1)) / (m + 1), the taps' sum being m + 1
__device__ __forceinline__ float sg_tap(int d, int m) {
  return (float)(m + 1 - (d < 0 ? -d : d)) / (float)((m + 1) * (m + 1));
}

// one frame of one row: s smoothed over time (taps read from the mask) then over frequency (in LDS), Y = X s laid out
// with its Hermitian half, inverse FFT, 1 / 1024, window -> frames [B][F][1024]
__global__ void __launch_bounds__(SG_TB) k_sg_back(const float2* __restrict__ X, const unsigned char* __restrict__ mask,
                                                   int F, const float* __restrict__ strength, int nf, int nt,
                                                   const float* __restrict__ tab, float* __restrict__ frames) {
  __shared__ float ar[SG_N], ai[SG_N], br[SG_N], bi[SG_N];
  __shared__ float us[SG_BINS + 2 * SG_MAX_HALF];
  const int b = blockIdx.y, t = blockIdx.x;
  const float p = strength[b];
  if (p < 0.f) return;
  const float2* tw = reinterpret_cast<const float2*>(tab);
  const float* win = tab + 2 * SG_N;
  const float off = 1.f - p;  // s where the mask is clear: p * (0 - 1) + 1
  const unsigned char* mb = mask + (long long)b * F * SG_BINS;
  for (int i = threadIdx.x; i < SG_BINS + 2 * nf; i += SG_TB) {
    const int f = i - nf;
    float u = 0.f;
    if (f >= 0 && f < SG_BINS) {
      const int lo = t - nt < 0 ? 0 : t - nt, hi = t + nt > F - 1 ? F - 1 : t + nt;
      for (int q = lo; q <= hi; ++q) u = fmaf(sg_tap(q - t, nt), mb[(long long)q * SG_BINS + f] ? 1.f : off, u);
    }
    us[i] = u;
  }
  __syncthreads();
  const float2* Xf = X + ((long long)b * F + t) * SG_BINS;
  for (int f = threadIdx.x; f < SG_BINS; f += SG_TB) {
    float sm = 0.f;
    for (int d = -nf; d <= nf; ++d) sm = fmaf(sg_tap(d, nf), us[f + nf + d], sm);
    const float2 v = Xf[f];
    const float re = v.x * sm, im = (f == 0 || f == SG_N / 2) ? 0.f : v.y * sm;  // c2r ignores those two
    ar[f] = re;
    ai[f] = im;
    if (f > 0 && f < SG_N / 2) {
      ar[SG_N - f] = re;
      ai[SG_N - f] = -im;
    }
  }
  __syncthreads();
  fft1024<true>(ar, ai, br, bi, tw);
  float* fr = frames + ((long long)b * F + t) * SG_N;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = threadIdx.x + 256 * r;
    fr[i] = br[i] * (1.f / SG_N) * win[i];
  }
}

// y[j], j < n_out: the frames that cover padded sample j + 512, summed in ascending frame order, over the same sum of
// the squared window; [n_out, n) zeros. A row that is not gated is copied through.
__global__ void __launch_bounds__(SG_TB) k_sg_ola(const float* __restrict__ frames, int F, long long n,
                                                  const float* __restrict__ strength, const float* __restrict__ tab,
                                                  const float* __restrict__ x, long long ldx, float* __restrict__ y,
                                                  long long ldy) {
  const int b = blockIdx.y;
  const long long j = (long long)blockIdx.x * SG_TB + threadIdx.x;
  if (j >= n) return;
  if (strength[b] < 0.f) {
    y[b * ldy + j] = x[b * ldx + j];
    return;
  }
  const long long n_out = (long long)SG_HOP * (F - 1);
  float v = 0.f;
  if (j < n_out) {
    const float* win = tab + 2 * SG_N;
    const long long pz = j + SG_N / 2;
    const int th = (int)(pz / SG_HOP);
    const int lo = th - 3 < 0 ? 0 : th - 3, hi = th > F - 1 ? F - 1 : th;
    float acc = 0.f, env = 0.f;
    for (int t = lo; t <= hi; ++t) {
      const int o = (int)(pz - (long long)t * SG_HOP);
      acc += frames[((long long)b * F + t) * SG_N + o];
      env = fmaf(win[o], win[o], env);
    }
    v = acc / env;
  }
  y[b * ldy + j] = v;
}
}  // namespace

void sg_tables(float* tab) {
  for (int m = 0; m < SG_N; ++m) {
    const double a = -2.0 * M_PI * (double)m / (double)SG_N;
    tab[2 * m] = (float)std::cos(a);
    tab[2 * m + 1] = (float)std::sin(a);
    tab[2 * SG_N + m] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)m / (double)SG_N));
  }
}

hipError_t spectral_gate(const float* x, long long ldx, long long n, const float* strength, int nf, int nt,
                         const float* tab, float* X, float* db, unsigned char* mask, float* frames, float* y,
                         long long ldy, unsigned char* mask_out, int B, hipStream_t s) {
  const int F = (int)sg_frames(n);
  const dim3 per_frame(F, B);
  hipLaunchKernelGGL(k_sg_forward, per_frame, dim3(SG_TB), 0, s, x, ldx, n, F, strength, tab,
                     reinterpret_cast<float2*>(X), db);
  hipLaunchKernelGGL(k_sg_stats, dim3((SG_BINS + 63) / 64, B), dim3(SG_TB), 0, s, db, F, strength, mask, mask_out);
  hipLaunchKernelGGL(k_sg_back, per_frame, dim3(SG_TB), 0, s, reinterpret_cast<const float2*>(X), mask, F, strength, nf,
                     nt, tab, frames);
  hipLaunchKernelGGL(k_sg_ola, dim3((unsigned)((n + SG_TB - 1) / SG_TB), B), dim3(SG_TB), 0, s, frames, F, n, strength,
                     tab, x, ldx, y, ldy);
  return hipGetLastError();
}

}  // namespace rvcx
