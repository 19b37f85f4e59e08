// The whole-utterance pipeline's sample-domain DSP on device: the (b, a) high-pass filtfilt and the odd extension the
// second-order-section form shares, peak normalisation, the long-input split points and the RMS volume envelope.
#include <algorithm>
#include <cmath>

#include "device_util.h"
#include "pipeline_kernels.h"

// a product and a sum fuse within one expression only, never across statements
#pragma clang fp contract(on)

namespace rvcx {

// scipy.signal.filtfilt(b, a, x) with padtype='odd', padlen = 3*max(len(a), len(b)) (pipeline.py:439),
// lfilter in direct form II transposed, fp64. The 5th-order 48 Hz high-pass has poles at |p| <= 0.9942
// and a highly non-normal DF2T state matrix (||F^256|| ~ 4e7), so chunk-state propagation
// (s_{c+1} = F^L s_c + e_c) is numerically unstable. Instead each chunk of IIR_L outputs re-runs
// IIR_W samples of history from a zero state (||F^10240|| ~ 1e-18, so the truncated history is below
// fp64 resolution); chunks that reach the signal start run from lfilter_zi * x[0] exactly as scipy.
// Measured vs scipy on the 13.5 s reference clip: max |diff| 3.4e-8 (below the fp32 ulp the models see).
constexpr int IIR_L = 512;
constexpr int IIR_W = 8192;  // ||F^8192|| ~ 2e-14: truncated history far below the DF2T's own rounding noise

struct IirCoef {
  double b[IIR_MAXO + 1], a[IIR_MAXO + 1], zi[IIR_MAXO];
  int order;
};

template <int O>
__device__ __forceinline__ double iir_step(const IirCoef& c, double* z, double x) {
  const double y = c.b[0] * x + z[0];
#pragma unroll
  for (int i = 0; i < O - 1; ++i) z[i] = c.b[i + 1] * x + z[i + 1] - c.a[i + 1] * y;
  z[O - 1] = c.b[O] * x - c.a[O] * y;
  return y;
}

// odd extension of x by padlen on both sides (scipy _arraytools.odd_ext)
__global__ void k_odd_ext(const double* x, long long n, int padlen, double* e) {
  const long long ne = n + 2 * padlen;
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < ne; j += (long long)gridDim.x * blockDim.x) {
    const long long k = j - padlen;
    double v;
    if (k < 0) v = 2.0 * x[0] - x[-k];
    else if (k >= n) v = 2.0 * x[n - 1] - x[2 * (n - 1) - k];
    else v = x[k];
    e[j] = v;
  }
}

// one pass of lfilter over seq (read reversed when rev): chunk ch writes outputs [ch*L, ch*L+L)
template <int O>
__global__ void k_iir_warm(const IirCoef c, const double* seq, long long ne, int rev, double* out) {
  const long long ch = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long nch = (ne + IIR_L - 1) / IIR_L;
  if (ch >= nch) return;
  const long long j0 = ch * IIR_L, j1 = min(ne, j0 + IIR_L);
  long long js = j0 - IIR_W;
  double z[O];
  auto at = [&](long long j) { return rev ? seq[ne - 1 - j] : seq[j]; };
  if (js <= 0) {
    js = 0;
    const double x0 = at(0);
#pragma unroll
    for (int i = 0; i < O; ++i) z[i] = c.zi[i] * x0;
  } else {
#pragma unroll
    for (int i = 0; i < O; ++i) z[i] = 0.0;
  }
  // warm-up over history (no outputs), 16 inputs fetched per batch ahead of the recurrence
  constexpr int NB = 16;
  long long j = js;
  for (; j + NB <= j0; j += NB) {
    double xb[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) xb[i] = at(j + i);
#pragma unroll
    for (int i = 0; i < NB; ++i) (void)iir_step<O>(c, z, xb[i]);
  }
  for (; j < j0; ++j) (void)iir_step<O>(c, z, at(j));
  for (; j + NB <= j1; j += NB) {
    double xb[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) xb[i] = at(j + i);
#pragma unroll
    for (int i = 0; i < NB; ++i) out[j + i] = iir_step<O>(c, z, xb[i]);
  }
  for (; j < j1; ++j) out[j] = iir_step<O>(c, z, at(j));
}

// audio_pad[k] = y[reflect(k - t_pad)] with y the filtfilt output (backward pass result yb reversed, trimmed)
__global__ void k_filt_pad(const double* yb, long long ne, int padlen, long long n, long long t_pad, double* pad64,
                           float* pad32) {
  const long long m = n + 2 * t_pad;
  for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < m; k += (long long)gridDim.x * blockDim.x) {
    long long j = k - t_pad;
    if (j < 0) j = -j;
    if (j >= n) j = 2 * (n - 1) - j;
    const double v = yb[ne - 1 - (j + padlen)];
    if (pad64) pad64[k] = v;
    pad32[k] = (float)v;
  }
}

hipError_t filtfilt_pad(const double* x, long long n, const double* b, const double* a, const double* zi, int order,
                        long long t_pad, double* ws, double* pad64, float* pad32, hipStream_t s) {
  if (order < 1 || order > IIR_MAXO) return hipErrorInvalidValue;
  const int padlen = 3 * (order + 1);
  if (n <= padlen || t_pad >= n) return hipErrorInvalidValue;
  IirCoef c;
  c.order = order;
  for (int i = 0; i <= order; ++i) {
    c.b[i] = b[i];
    c.a[i] = a[i];
  }
  for (int i = 0; i < order; ++i) c.zi[i] = zi[i];
  const long long ne = n + 2 * padlen;
  const long long nch = (ne + IIR_L - 1) / IIR_L;
  double* ext = ws;
  double* yf = ext + ne;
  double* yb = yf + ne;
  hipLaunchKernelGGL(k_odd_ext, dim3(nblocks(ne)), dim3(TB), 0, s, x, n, padlen, ext);
  const unsigned g = (unsigned)((nch + 63) / 64);
  for (int rev = 0; rev < 2; ++rev) {
    const double* in = rev ? yf : ext;
    double* o = rev ? yb : yf;
    switch (order) {
#define RVCX_IIR_CASE(O_) \
  case O_: hipLaunchKernelGGL(k_iir_warm<O_>, dim3(g), dim3(64), 0, s, c, in, ne, rev, o); break;
      RVCX_IIR_CASE(1) RVCX_IIR_CASE(2) RVCX_IIR_CASE(3) RVCX_IIR_CASE(4)
      RVCX_IIR_CASE(5) RVCX_IIR_CASE(6) RVCX_IIR_CASE(7) RVCX_IIR_CASE(8)
#undef RVCX_IIR_CASE
      default: return hipErrorInvalidValue;
    }
  }
  hipLaunchKernelGGL(k_filt_pad, dim3(nblocks(n + 2 * t_pad)), dim3(TB), 0, s, yb, ne, padlen, n, t_pad, pad64,
                     pad32);
  return hipGetLastError();
}

hipError_t filtfilt_sos_pad(const SosPlan& p, int order, const double* x, long long n, long long t_pad, double* ws,
                            double* pad64, float* pad32, hipStream_t s) {
  const int padlen = 3 * (order + 1);
  if (n <= padlen || t_pad >= n || p.nsec < 1) return hipErrorInvalidValue;
  const long long ne = n + 2 * padlen;
  if (!p.casc) return hipErrorInvalidValue;
  double* ext = ws;
  hipLaunchKernelGGL(k_odd_ext, dim3(nblocks(ne)), dim3(TB), 0, s, x, n, padlen, ext);
  return casc_filtfilt_pad(p, ext, ne, padlen, n, t_pad, ext + ne, pad64, pad32, s);
}

size_t filtfilt_sos_ws_doubles(long long n, int order) {
  const long long ne = n + 2 * 3 * (order + 1);
  return (size_t)(3 * ne) + casc_ws_doubles(ne, 64);
}

size_t filtfilt_ws_doubles(long long n, int order) {
  const long long ne = n + 2 * 3 * (order + 1);
  return (size_t)(3 * ne);
}

// peak normalisation (pipeline.py:550-552): m = max|x| / 0.99 ; if m > 1: x /= m. Fused with the trim copy
// (pipeline.py:494 audio_opt slices): dst = src / m read from the un-trimmed buffer. Two launches for all B rows
// (row b's first nv[b] samples) and no fill: each absmax block writes its own maximum to ws[row][block], the scale
// pass reduces those <= 256 partials per block before it scales (no atomics, nothing to zero between calls).
constexpr int PEAK_BLOCKS = 256;
__global__ void k_absmax(const float* x, Len nv, long long ldx, float* part) {
  __shared__ float wm[TB / 64];
  x += blockIdx.y * ldx;
  const long long n = nv[blockIdx.y];
  float m = 0.f;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    m = fmaxf(m, fabsf(x[i]));
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, wm[w]);
    part[blockIdx.y * PEAK_BLOCKS + blockIdx.x] = m;
  }
}
__global__ void k_peak_scale(const float* src, long long lds, float* dst, long long ldd, Len nv, const float* part,
                             int nparts) {
  __shared__ float wm[TB / 64];
  src += blockIdx.y * lds;
  dst += blockIdx.y * ldd;
  const long long n = nv[blockIdx.y];
  float m = threadIdx.x < nparts ? part[blockIdx.y * PEAK_BLOCKS + threadIdx.x] : 0.f;
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  m = wm[0];
  for (int w = 1; w < TB / 64; ++w) m = fmaxf(m, wm[w]);
  m = m / 0.99f;
  const bool scale = m > 1.f;
  if (!scale && src == dst) return;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    dst[i] = scale ? src[i] / m : src[i];
}
hipError_t peak_normalize(const float* src, long long lds, float* dst, long long ldd, Len n, long long n_max, float* ws,
                          hipStream_t s, int B) {
  if (n_max <= 0 || B < 1) return hipSuccess;
  if (n_max >= (1LL << 31)) return hipErrorInvalidValue;
  const int nparts = (int)std::min<long long>(PEAK_BLOCKS, (n_max + TB - 1) / TB);
  hipLaunchKernelGGL(k_absmax, dim3(nparts, B), dim3(TB), 0, s, src, n, lds, ws);
  hipLaunchKernelGGL(k_peak_scale, dim3(std::min(nblocks(n_max), 4096u), B), dim3(TB), 0, s, src, lds, dst, ldd, n, ws,
                     nparts);
  return hipGetLastError();
}
size_t peak_normalize_ws_floats(int B) { return (size_t)B * PEAK_BLOCKS; }

// ------------------------------------------------------------------ long-input split points
// Pipeline.pipeline opt_ts search (rvc/infer/pipeline.py:440-452): with xp = reflect-pad(x, w/2),
// audio_sum[p] = sum_{i<w} xp[p+i] accumulated in i order (numpy's `audio_sum += audio_pad[i:i-w]`,
// so the fp64 result is bit-identical), then for every t = t_center, 2 t_center, ... < n the split
// is t - t_query + first argmin |audio_sum[t - t_query : t + t_query]|.
__global__ void k_window_sum(const double* x, long long n, int w, double* sum) {
  const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (p >= n) return;
  const long long h = w / 2;
  double acc = 0.0;
  for (int i = 0; i < w; ++i) {
    long long q = p + i - h;
    if (q < 0) q = -q;
    if (q >= n) q = 2 * (n - 1) - q;
    acc += x[q];
  }
  sum[p] = acc;
}
__global__ void k_split_argmin(const double* sum, long long n, long long t_center, long long t_query,
                               long long* ts) {
  const long long t = t_center * (blockIdx.x + 1);
  const long long lo = t - t_query;
  const long long hi = t + t_query < n ? t + t_query : n;
  double bv = INFINITY;
  long long bi = hi;
  for (long long p = lo + threadIdx.x; p < hi; p += blockDim.x) {
    const double v = fabs(sum[p]);
    if (v < bv) {  // ascending p per thread: keeps the first minimum
      bv = v;
      bi = p;
    }
  }
  __shared__ double sv[TB];
  __shared__ long long si[TB];
  sv[threadIdx.x] = bv;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int o = TB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double v2 = sv[threadIdx.x + o];
      const long long i2 = si[threadIdx.x + o];
      if (v2 < sv[threadIdx.x] || (v2 == sv[threadIdx.x] && i2 < si[threadIdx.x])) {
        sv[threadIdx.x] = v2;
        si[threadIdx.x] = i2;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) ts[blockIdx.x] = si[0];
}
hipError_t split_points(const double* x, long long n, int window, long long t_center, long long t_query,
                        double* sum_ws, long long* ts, int nts, hipStream_t s) {
  hipLaunchKernelGGL(k_window_sum, dim3(nblocks(n)), dim3(TB), 0, s, x, n, window, sum_ws);
  if (nts > 0) hipLaunchKernelGGL(k_split_argmin, dim3(nts), dim3(TB), 0, s, sum_ws, n, t_center, t_query, ts);
  return hipGetLastError();
}

// ------------------------------------------------------------------ volume envelope
// AudioProcessor.change_rms (rvc/infer/pipeline.py:35-82): librosa.feature.rms (center=True, zero pad
// frame/2, mean |x|^2 per frame, sqrt) of source and target, both linearly interpolated
// (F.interpolate mode='linear', align_corners=False) to the target length, then
// y *= rms1^(1-rate) * max(rms2, 1e-6)^(rate-1). One block per RMS frame, fp64 sums.
// One launch set for all rows (blockIdx.y = row): row b of x (stride ld) has nv[b] samples and 1 + nv[b] / hop frames,
// written at rms + b*ld_rms behind the row's 1 + n_before[b] / hop_before source frames (hop_before 0: none before).
// rate (optional): a row whose rate is exactly 1 is skipped.
template <class T>
__global__ void k_rms_frames(const T* x, long long ld, Len nv, int frame, int hop, float* rms, long long ld_rms,
                             Len n_before, int hop_before, const float* __restrict__ rate) {
  const int b = blockIdx.y;
  if (rate && rate[b] == 1.f) return;
  const long long n = nv[b];
  if ((long long)blockIdx.x >= 1 + n / hop) return;
  x += b * ld;
  rms += b * ld_rms + (hop_before ? 1 + n_before[b] / hop_before : 0);
  const long long start = (long long)blockIdx.x * hop - frame / 2;
  double acc = 0.0;
  for (int j = threadIdx.x; j < frame; j += blockDim.x) {
    const long long q = start + j;
    if (q >= 0 && q < n) {
      const double v = (double)x[q];
      acc += v * v;
    }
  }
  __shared__ double red[TB];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = TB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) rms[blockIdx.x] = (float)sqrt(red[0] / frame);
}
// librosa.feature.rms (center=True, zero pad frame/2) kept in fp64 for librosa.effects.split's power_to_db test
// (rvc/lib/tools/split_audio.py:19-24): rms[k] = sqrt(mean over the frame of x^2), frame k centred at k*hop.
__global__ void k_rms_frames_f64(const double* x, long long n, int frame, int hop, double* rms) {
  const long long start = (long long)blockIdx.x * hop - frame / 2;
  double acc = 0.0;
  for (int j = threadIdx.x; j < frame; j += blockDim.x) {
    const long long q = start + j;
    if (q >= 0 && q < n) acc += x[q] * x[q];
  }
  __shared__ double red[TB];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = TB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) rms[blockIdx.x] = sqrt(red[0] / frame);
}
hipError_t rms_frames_f64(const double* x, long long n, int frame, int hop, double* rms, int nframes, hipStream_t s) {
  if (frame <= 0 || hop <= 0 || nframes <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rms_frames_f64, dim3(nframes), dim3(TB), 0, s, x, n, frame, hop, rms);
  return hipGetLastError();
}
__device__ __forceinline__ float interp_linear(const float* r, int n_in, long long i, long long n_out) {
  const float scale = (float)n_in / (float)n_out;
  float src = scale * ((float)i + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  int i0 = (int)src;
  if (i0 > n_in - 1) i0 = n_in - 1;
  const int i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  float l1 = src - (float)i0;
  l1 = fminf(fmaxf(l1, 0.f), 1.f);
  return (1.f - l1) * r[i0] + l1 * r[i1];
}
// row b: its source frames at ws + b*ld_ws, then its target frames; rate_v (optional): the row's own rate, exactly 1 =
// the row is left untouched
__global__ void k_apply_rms(float* y, long long ld, Len n_y, const float* ws, long long ld_ws, Len n_src, int hop_src,
                            int hop_y, float rate, const float* __restrict__ rate_v) {
  const int b = blockIdx.y;
  if (rate_v) rate = rate_v[b];
  if (rate_v && rate == 1.f) return;
  const long long n = n_y[b];
  const int n1 = 1 + n_src[b] / hop_src, n2 = (int)(1 + n / hop_y);
  y += b * ld;
  const float* r1 = ws + b * ld_ws;
  const float* r2 = r1 + n1;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float a = interp_linear(r1, n1, i, n);
    const float c = fmaxf(interp_linear(r2, n2, i, n), 1e-6f);
    y[i] = y[i] * (powf(a, 1.f - rate) * powf(c, rate - 1.f));
  }
}
int rms_frame_count(long long n, int sr) { return (int)(1 + n / (sr / 2)); }
template <class S>
hipError_t change_rms(const S* src, long long ld_src, Len n_src, long long n_src_max, int sr_src, float* y,
                      long long ld_y, Len n_y, long long n_y_max, int sr_y, float rate, const float* rate_v, float* ws,
                      hipStream_t s, int B) {
  if (B < 1) return hipSuccess;
  if (n_src_max >= (1LL << 31) || n_y_max >= (1LL << 31)) return hipErrorInvalidValue;
  const int n1 = rms_frame_count(n_src_max, sr_src), n2 = rms_frame_count(n_y_max, sr_y);
  const long long ld_ws = n1 + n2;
  hipLaunchKernelGGL(k_rms_frames<S>, dim3(n1, B), dim3(TB), 0, s, src, ld_src, n_src, sr_src / 2 * 2, sr_src / 2, ws,
                     ld_ws, Len(0), 0, rate_v);
  hipLaunchKernelGGL(k_rms_frames<float>, dim3(n2, B), dim3(TB), 0, s, (const float*)y, ld_y, n_y, sr_y / 2 * 2,
                     sr_y / 2, ws, ld_ws, n_src, sr_src / 2, rate_v);
  hipLaunchKernelGGL(k_apply_rms, dim3(std::min(nblocks(n_y_max), 4096u), B), dim3(TB), 0, s, y, ld_y, n_y, ws, ld_ws,
                     n_src, sr_src / 2, sr_y / 2, rate, rate_v);
  return hipGetLastError();
}
template hipError_t change_rms<double>(const double*, long long, Len, long long, int, float*, long long, Len, long long,
                                       int, float, const float*, float*, hipStream_t, int);
template hipError_t change_rms<float>(const float*, long long, Len, long long, int, float*, long long, Len, long long,
                                      int, float, const float*, float*, hipStream_t, int);

}  // namespace rvcx
