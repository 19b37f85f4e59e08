// Non-GEMM kernels of the FCPE pitch network (rvc/lib/predictors/FCPE.py): the input stack's GroupNorm + LeakyReLU,
// the Conformer module's GLU + depthwise conv + Swish, the cents decoders and FCPEF0Predictor.post_process (the STFT
// magnitude of its mel is rmvpe_aux.hip's, shared with RMVPE). The Performer attention is performer_attn.hip; the convs
// and linears run on the implicit-GEMM family. The kernels that pad or reduce over time (GroupNorm, the depthwise conv, the mel's padding
// and repeated last frame) take B streams of one length per launch, grid z (or y) = stream, each stream on its own
// rows; the row-wise ones (the decoders) run on the B F rows of all streams. For utterances of different lengths each
// of them also takes a device array of the streams' own frame counts inside slots of one length (fcpe_forward_v),
// indexed by the grid's stream index, so the length is one scalar load and every branch on it is the workgroup's.
#include <algorithm>
#include <cmath>

#include "device_util.h"
#include "fcpe_kernels.h"

namespace rvcx {

namespace {

__device__ __forceinline__ float sigmoidf(float z) { return 1.f / (1.f + expf(-z)); }

// y[b][i] = x[b ldx + i - pad_l] for pad_l <= i < pad_l + n, else 0, i < ldy: the zero padding STFT.get_mel falls back
// to when the reflection does not fit (FCPE.py:138), per stream
__global__ void k_fcpe_zero_pad(const float* x, int n, int pad_l, long long ldx, float* y, long long ldy) {
  x += blockIdx.y * ldx;
  y += blockIdx.y * ldy;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < ldy; i += (long long)gridDim.x * blockDim.x)
    y[i] = (i >= pad_l && i < (long long)pad_l + n) ? x[i - pad_l] : 0.f;
}

// mel [B][F][C]: row F - 1 of every stream = a copy of its own row F - 2 (Wav2Mel.extract_mel's appended frame,
// FCPE.py:808-812)
__global__ void k_fcpe_dup_last(float* mel, int F, int C) {
  float* m = mel + (long long)blockIdx.x * F * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) m[(long long)(F - 1) * C + c] = m[(long long)(F - 2) * C + c];
}

// The ragged form: stream b has Fv[b] <= F frames in its F-row slot. Row Fv[b] - 1 = a copy of row Fv[b] - 2 (written
// by nobody here), rows Fv[b] .. F - 1 zero. One workgroup per (row from Fv[b] - 1 on, stream).
__global__ void k_fcpe_mel_tail_v(float* mel, const int* Fv, int F, int C) {
  const int Fb = Fv[blockIdx.y], t = Fb - 1 + (int)blockIdx.x;
  if (t >= F) return;
  float* m = mel + (long long)blockIdx.y * F * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x)
    m[(long long)t * C + c] = t == Fb - 1 ? m[(long long)(Fb - 2) * C + c] : 0.f;
}

// GroupNorm(G, C) over time-major x [T][C] in place, then LeakyReLU(slope) (FCPE.py:626-630: the statistics of a
// group run over its C / G channels x T frames). Two launches: k_gn_stats sums each of GN_TCHUNKS time chunks of a
// group in fp64 (a fixed tree over the workgroup) into ws [G][GN_TCHUNKS][2]; k_gn_apply adds the chunks in chunk
// order (every thread the same sequence: no atomics, run-to-run bit identical) and normalises. grid z = stream: B
// sequences of T rows back to back, the statistics per (stream, group), ws [B][G][GN_TCHUNKS][2]. With Tv, stream b
// has Tv[b] <= T rows in its T-row slot (one scalar load per workgroup): the chunks are those of Tv[b] rows, so the
// sums are the ones a call on that stream alone forms, and k_gn_apply sets the slot's rows from Tv[b] on to zero.
constexpr int GN_TCHUNKS = FCPE_GN_CHUNKS;
__global__ __launch_bounds__(256) void k_gn_stats(const float* x, int Ts, int C, int G, double* ws, const int* Tv) {
  __shared__ double s1[256], s2[256];
  const int g = blockIdx.y, cg = C / G, c0 = g * cg;
  const int T = Tv ? Tv[blockIdx.z] : Ts;
  x += (long long)blockIdx.z * Ts * C;
  ws += (long long)blockIdx.z * G * GN_TCHUNKS * 2;
  const int per = (T + GN_TCHUNKS - 1) / GN_TCHUNKS;
  const int t_lo = min(T, (int)blockIdx.x * per), t_hi = min(T, t_lo + per);
  const long long n = (long long)(t_hi - t_lo) * cg;
  double a = 0.0, b = 0.0;
  for (long long i = threadIdx.x; i < n; i += blockDim.x) {
    const double v = x[(t_lo + i / cg) * C + c0 + (int)(i % cg)];
    a += v;
    b += v * v;
  }
  s1[threadIdx.x] = a;
  s2[threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s1[threadIdx.x] += s1[threadIdx.x + o];
      s2[threadIdx.x] += s2[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ws[((long long)g * GN_TCHUNKS + blockIdx.x) * 2] = s1[0];
    ws[((long long)g * GN_TCHUNKS + blockIdx.x) * 2 + 1] = s2[0];
  }
}
__global__ __launch_bounds__(256) void k_gn_apply(float* x, int Ts, int C, int G, const double* ws, const float* gamma,
                                                  const float* beta, float eps, float slope, const int* Tv) {
  const int g = blockIdx.y, cg = C / G, c0 = g * cg;
  const int T = Tv ? Tv[blockIdx.z] : Ts;
  const long long n = (long long)T * cg, ns = (long long)Ts * cg;
  x += (long long)blockIdx.z * Ts * C;
  ws += (long long)blockIdx.z * G * GN_TCHUNKS * 2;
  double a = 0.0, b = 0.0;
  for (int k = 0; k < GN_TCHUNKS; ++k) {
    a += ws[((long long)g * GN_TCHUNKS + k) * 2];
    b += ws[((long long)g * GN_TCHUNKS + k) * 2 + 1];
  }
  const double mean = a / (double)n;
  const double var = fmax(b / (double)n - mean * mean, 0.0);
  const float mu = (float)mean, rstd = (float)(1.0 / sqrt(var + (double)eps));
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < ns; i += (long long)gridDim.x * blockDim.x) {
    const int c = c0 + (int)(i % cg);
    float* p = x + (i / cg) * C + c;
    if (i >= n) {  // a row past the stream's own end
      *p = 0.f;
      continue;
    }
    const float v = (*p - mu) * rstd * gamma[c] + beta[c];
    *p = v > 0.f ? v : v * slope;
  }
}

// ConformerConvModule's middle (FCPE.py:339-344) as one kernel over the 1x1 conv's output x [T][2 C2]:
//   g[t][c] = x[t][c] sigmoid(x[t][C2 + c])                         GLU (formed while the tile is loaded)
//   y[t][c] = swish(b[c] + sum_k w[k][c] g[t + k - pad][c])         depthwise conv, zero padding, Swish
// One workgroup per (64 channels, 32 output frames, stream): the GLU'd rows t0 - pad .. t0 + 31 + K - 1 - pad sit in
// LDS. grid z = stream (B sequences of T rows back to back): the zero padding is each stream's own, t outside [0, T).
// With Tv, stream b ends at row Tv[b] <= T of its T-row slot: workgroups from there on exit (before the barrier: the
// condition is the workgroup's), taps from there on read zero.
constexpr int DW_T = 32, DW_MAXK = 64;
__global__ __launch_bounds__(256) void k_glu_dw_swish(const float* x, int Ts, int C2, const float* w, const float* b,
                                                       int K, int pad, float* y, const int* Tv) {
  __shared__ float g[(DW_T + DW_MAXK - 1) * 64];
  const int cl = threadIdx.x & 63, tg = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const int t0 = blockIdx.y * DW_T;
  const int rows = DW_T + K - 1;
  const int T = Tv ? Tv[blockIdx.z] : Ts;
  if (t0 >= T) return;
  x += (long long)blockIdx.z * Ts * 2 * C2;
  y += (long long)blockIdx.z * Ts * C2;
  for (int i = tg; i < rows; i += 4) {
    const int t = t0 - pad + i;
    float v = 0.f;
    if (t >= 0 && t < T) {
      const float* xr = x + (long long)t * 2 * C2;
      v = xr[c] * sigmoidf(xr[C2 + c]);
    }
    g[i * 64 + cl] = v;
  }
  __syncthreads();
  const float bias = b[c];
#pragma unroll
  for (int j = 0; j < DW_T / 4; ++j) {
    const int r = tg * (DW_T / 4) + j;
    if (t0 + r >= T) break;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(w[k * C2 + c], g[(r + k) * 64 + cl], acc);
    const float v = acc + bias;
    y[(long long)(t0 + r) * C2 + c] = v * sigmoidf(v);
  }
}

// cents_local_decoder / cents_decoder + cent_to_f0 (FCPE.py:683-714): one wave per frame of salience [F][nb].
//   mode 0 "local_argmax": the first maximal bin, its +-4 window with every index clamped to [0, nb - 1] (a clamped
//          index counts once per window slot, as torch.gather does), cents = sum(ci y) / sum(y) over the 9 slots
//   mode 1 "argmax": cents = sum(ci y) / sum(y) over all bins
// f0 = 10 * 2^(cents / 1200), 0 where max <= threshold (the reference's -inf cents). The fp32 products are summed in
// fp64 and the quotient is taken in fp32; f0 is written as the exact fp32 value in fp64.
__device__ __forceinline__ void decode_frame(const float* s, int nb, const float* cent, float thr, int mode,
                                             double* f0) {
  const int lane = threadIdx.x & 63;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  double num = 0.0, den = 0.0;
  for (int k = lane; k < nb; k += 64) {
    const float v = s[k];
    if (v > best) {
      best = v;
      bi = k;
    }
    num += (double)(cent[k] * v);
    den += (double)v;
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
  num = wave_sum(num);
  den = wave_sum(den);
  if (lane != 0) return;
  // a frame with no value above -inf (all NaN) leaves bi at INT_MAX, and the window's `bi - 4 + j` then overflows:
  // the compiler folds the clamp into max(bi, 4 - j) + (j - 4), which wraps to an index far below the row
  bi = min(bi, nb - 1);
  if (mode == 0) {
    num = 0.0;
    den = 0.0;
    for (int j = 0; j < 9; ++j) {
      const int k = min(max(bi - 4 + j, 0), nb - 1);
      num += (double)(cent[k] * s[k]);
      den += (double)s[k];
    }
  }
  const float cents = (float)num / (float)den;
  *f0 = best <= thr ? 0.0 : (double)(10.f * exp2f(cents / 1200.f));
}
__global__ void k_fcpe_decode(const float* sal, int F, int nb, const float* cent, float thr, int mode, double* f0) {
  const int f = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (f >= F) return;
  decode_frame(sal + (long long)f * nb, nb, cent, thr, mode, f0 + f);
}
// grid y = stream: its Fv[b] frames of the F-row slot, f0 rows of stride ldf
__global__ void k_fcpe_decode_v(const float* sal, const int* Fv, int F, int nb, const float* cent, float thr, int mode,
                                double* f0, long long ldf) {
  const int f = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), b = blockIdx.y;
  if (f >= Fv[b]) return;
  decode_frame(sal + ((long long)b * F + f) * nb, nb, cent, thr, mode, f0 + b * ldf + f);
}

// FCPEF0Predictor.post_process (FCPE.py:877-902) on a raw track f0 [F]: e[i] = f0[nearest(i)] for i < n
// (repeat_expand: torch's nearest interpolation), then np.interp through the frames with e != 0, the first / last
// of them held at the ends; zeros when there is none.
__device__ __forceinline__ int nearest_src(int i, int F, int n) {  // ATen nearest_idx (UpSample.h)
  if (n == F) return i;
  if (n == 2 * F) return i >> 1;
  const float scale = (float)F / (float)n;
  return min((int)floorf((float)i * scale), F - 1);
}

// prev[i] / next[i]: the nearest index <= i / >= i with e != 0 (-1 / n when none). One workgroup; thread k owns
// the segment [k L, (k + 1) L).
__global__ __launch_bounds__(1024) void k_fcpe_voiced_links(const double* f0, int F, int n, int* prev, int* next) {
  __shared__ int last[1024], first[1024];
  const int L = (n + 1023) / 1024;
  const int lo = min(n, (int)threadIdx.x * L), hi = min(n, lo + L);
  int la = -1, fi = n;
  for (int i = lo; i < hi; ++i)
    if (f0[nearest_src(i, F, n)] != 0.0) {
      la = i;
      if (fi == n) fi = i;
    }
  last[threadIdx.x] = la;
  first[threadIdx.x] = fi;
  __syncthreads();
  int carry = -1;
  for (int k = (int)threadIdx.x - 1; k >= 0 && carry < 0; --k) carry = last[k];
  for (int i = lo; i < hi; ++i) {
    if (f0[nearest_src(i, F, n)] != 0.0) carry = i;
    prev[i] = carry;
  }
  carry = n;
  for (int k = (int)threadIdx.x + 1; k < 1024 && carry == n; ++k) carry = first[k];
  for (int i = hi - 1; i >= lo; --i) {
    if (f0[nearest_src(i, F, n)] != 0.0) carry = i;
    next[i] = carry;
  }
}

__global__ void k_fcpe_interp(const double* f0, int F, int n, const int* prev, const int* next, double hop, double sr,
                              double* out) {
#pragma clang fp contract(off)  // numpy rounds every product and sum separately
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int p = prev[i], q = next[i];
  double v;
  if (p < 0 && q >= n) {
    v = 0.0;
  } else if (p < 0) {
    v = f0[nearest_src(q, F, n)];
  } else if (q >= n || p == i) {
    v = f0[nearest_src(p, F, n)];
  } else {
    // np.interp: slope (x - xp[j]) + fp[j] with xp = hop / sr * index (time_org), x = i * hop / sr (time_frame).
    // At a voiced frame (p == i, above) the value itself is returned; np.interp's x and xp there can differ by an
    // ulp, in which case it interpolates from the neighbouring segment: a difference of ~1e-16 relative
    const double fp0 = f0[nearest_src(p, F, n)], fp1 = f0[nearest_src(q, F, n)];
    const double step = hop / sr;
    const double x0 = step * (double)p, x1 = step * (double)q, xx = ((double)i * hop) / sr;
    const double slope = (fp1 - fp0) / (x1 - x0);
    v = slope * (xx - x0) + fp0;
  }
  out[i] = v;
}

}  // namespace

hipError_t fcpe_zero_pad(const float* x, int n, int pad_l, long long ldx, float* y, long long ldy, int B,
                         hipStream_t s) {
  if (n < 1 || pad_l < 0 || ldy < (long long)pad_l + n || B < 1 || B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fcpe_zero_pad, dim3(std::min(nblocks(ldy), 2048u), B), dim3(TB), 0, s, x, n, pad_l, ldx, y, ldy);
  return hipGetLastError();
}

hipError_t fcpe_dup_last_frame(float* mel, int B, int F, int C, hipStream_t s) {
  if (B < 1 || F < 2 || C < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fcpe_dup_last, dim3(B), dim3(TB), 0, s, mel, F, C);
  return hipGetLastError();
}

hipError_t fcpe_mel_tail_v(float* mel, int B, const int* Fv, int F, int F_min, int C, hipStream_t s) {
  if (B < 1 || B > 65535 || F_min < 2 || F < F_min || C < 1 || !Fv) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fcpe_mel_tail_v, dim3(F - F_min + 1, B), dim3(TB), 0, s, mel, Fv, F, C);
  return hipGetLastError();
}

hipError_t groupnorm_lrelu(float* x, int T, int C, int G, const float* gamma, const float* beta, float eps, float slope,
                           double* ws, hipStream_t s, int B, const int* Tv) {
  if (T < 1 || G < 1 || C % G || !ws || B < 1 || B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gn_stats, dim3(GN_TCHUNKS, G, B), dim3(256), 0, s, x, T, C, G, ws, Tv);
  const long long n = (long long)T * (C / G);
  hipLaunchKernelGGL(k_gn_apply, dim3((unsigned)std::min<long long>((n + 255) / 256, 1024), G, B), dim3(256), 0, s, x, T,
                     C, G, ws, gamma, beta, eps, slope, Tv);
  return hipGetLastError();
}

hipError_t glu_dwconv_swish(const float* x, int T, int C2, const float* w, const float* b, int K, int pad, float* y,
                            hipStream_t s, int B, const int* Tv) {
  if (T < 1 || C2 % 64 || K < 1 || K > DW_MAXK || pad < 0 || pad >= K || B < 1 || B > 65535)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_glu_dw_swish, dim3(C2 / 64, (T + DW_T - 1) / DW_T, B), dim3(256), 0, s, x, T, C2, w, b, K, pad, y,
                     Tv);
  return hipGetLastError();
}

hipError_t fcpe_decode(const float* sal, int F, int nb, const float* cent, float thr, int mode, double* f0,
                       hipStream_t s) {
  if (F < 1 || nb < 1 || mode < 0 || mode > 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fcpe_decode, dim3((F + 3) / 4), dim3(256), 0, s, sal, F, nb, cent, thr, mode, f0);
  return hipGetLastError();
}

hipError_t fcpe_decode_v(const float* sal, int B, const int* Fv, int F, int nb, const float* cent, float thr, int mode,
                         double* f0, long long ldf, hipStream_t s) {
  if (B < 1 || B > 65535 || F < 1 || nb < 1 || mode < 0 || mode > 1 || ldf < F || !Fv) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fcpe_decode_v, dim3((F + 3) / 4, B), dim3(256), 0, s, sal, Fv, F, nb, cent, thr, mode, f0, ldf);
  return hipGetLastError();
}

hipError_t fcpe_post_process(const double* f0, int F, int n, int hop, int sr, int* links, double* out,
                             hipStream_t s) {
  if (F < 1 || n < 1 || hop < 1 || sr < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fcpe_voiced_links, dim3(1), dim3(1024), 0, s, f0, F, n, links, links + n);
  hipLaunchKernelGGL(k_fcpe_interp, dim3(nblocks(n)), dim3(TB), 0, s, f0, F, n, links, links + n, (double)hop,
                     (double)sr, out);
  return hipGetLastError();
}

}  // namespace rvcx
