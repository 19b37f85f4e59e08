// The file-level front and back door on device: sample decode, channel downmix and the polyphase FIR of
// scipy.signal.resample_poly (window ("kaiser", 5.0), padtype "constant") in one launch, for rows of different lengths.
#include <algorithm>

#include "resample_kernels.h"

// a product and a sum fuse within one expression only, never across statements
#pragma clang fp contract(on)

namespace rvcx {

namespace {

constexpr int RS_THREADS = 256;
// the staged input window of a block, in doubles: 64 KiB, what a launch takes without opting in to more
constexpr int RS_LDS_DOUBLES = 8192;

// h [L] -> hp [up][K] with hp[p][k] = h[p + k*up], zero past L: the taps of one output sample are contiguous
__global__ void k_resample_taps(const double* h, long long L, int up, int K, double* hp) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= (long long)up * K) return;
  const long long src = t / K + (t % K) * (long long)up;
  hp[t] = src < L ? h[src] : 0.0;
}

// frame i of a row as the mono fp64 sample the host loader computes: every channel scaled by 1 / (iinfo.max + 1),
// summed in channel order, divided by the channel count
__device__ __forceinline__ double decode_frame(const void* row, int dtype, int channels, long long i) {
  const long long e = i * channels;
  double s = 0.0;
  for (int c = 0; c < channels; ++c) {
    double v;
    if (dtype == 0) v = static_cast<const double*>(row)[e + c];
    else if (dtype == 1) v = (double)static_cast<const float*>(row)[e + c];
    else if (dtype == 2) v = (double)static_cast<const int16_t*>(row)[e + c] * 0x1p-15;
    else v = (double)static_cast<const int32_t*>(row)[e + c] * 0x1p-31;
    s += v;
  }
  return channels == 1 ? s : s / (double)channels;
}

// Block (bx, b) computes outputs [bx*J, bx*J + J) of row b. Output j sits at c = (j + n_pre_remove)*down - n_pre_pad
// of the zero-stuffed signal (c >= 0 for every j: n_pre_remove*down > half + n_pre_pad - down and half >= down or
// half == 0 with down == 1), so with ih = c / up and p = c % up
//   y[j] = sum_k x[ih - k] * hp[p][k],  k = K-1 .. 0  (ascending input index, one fixed order).
// The block's inputs [i_base, i_base + count) are decoded once into LDS as fp64, zeros outside [0, n). Lanes read
// the window at a stride of down/up doubles: conflict-free for ds_read_b64 when that is an odd integer (48 -> 16 kHz).
// UP1: one phase, so every lane reads the same tap and the read is wave-uniform.
template <bool UP1>
__global__ void __launch_bounds__(RS_THREADS)
k_resample_poly(const void* x, int dtype, int esize, int channels, const long long* n_rows, long long ldx, int up,
                int down, const double* hp, int K, long long n_pre_remove, long long n_pre_pad, double* y,
                long long ldy, const long long* n_out_rows, int J) {
  extern __shared__ double xs[];
  const int b = blockIdx.y;
  const long long n = n_rows[b], n_out = n_out_rows[b];
  const long long j0 = (long long)blockIdx.x * J;
  double* yr = y + (long long)b * ldy;
  const int tid = threadIdx.x;
  if (j0 >= n_out) {  // the row's tail: zeros up to ldy
    if (tid < J && j0 + tid < ldy) yr[j0 + tid] = 0.0;
    return;
  }
  const char* row = static_cast<const char*>(x) + (long long)b * ldx * channels * esize;
  const long long j_last = min(j0 + J, n_out) - 1;
  const long long i_base = ((j0 + n_pre_remove) * down - n_pre_pad) / up - (K - 1);
  const long long i_top = ((j_last + n_pre_remove) * down - n_pre_pad) / up;
  const int count = (int)(i_top - i_base + 1);
  for (int t = tid; t < count; t += RS_THREADS) {
    const long long i = i_base + t;
    xs[t] = (i >= 0 && i < n) ? decode_frame(row, dtype, channels, i) : 0.0;
  }
  __syncthreads();
  const long long j = j0 + tid;
  if (tid >= J || j >= ldy) return;
  if (j >= n_out) {
    yr[j] = 0.0;
    return;
  }
  const long long c = (j + n_pre_remove) * down - n_pre_pad;
  const long long ih = c / up;
  const double* w = UP1 ? hp : hp + (c - ih * up) * K;
  const double* xw = xs + (ih - i_base);
  double acc = 0.0;
  for (int k = K - 1; k >= 0; --k) acc = __builtin_fma(xw[-k], w[k], acc);
  yr[j] = acc;
}

}  // namespace

ResamplePlan resample_poly_plan(int up, int down, long long ntaps) {
  ResamplePlan p;
  const long long half = (ntaps - 1) / 2;
  p.K = (int)((ntaps + up - 1) / up);
  p.n_pre_pad = down - half % down;
  p.n_pre_remove = (half + p.n_pre_pad) / down;
  // outputs per block: as many as the block has threads while the window (J-1)*down/up + 1 + K fits
  long long J = RS_THREADS;
  const long long room = (long long)RS_LDS_DOUBLES - 1 - p.K;
  if (room < 0) {
    p.J = 0;
    return p;
  }
  J = std::min<long long>(J, room * up / down + 1);
  p.J = (int)J;
  p.window = (int)((J - 1) * down / up + 1 + p.K);
  return p;
}

hipError_t resample_poly_taps(const double* h, long long ntaps, int up, int K, double* hp, hipStream_t s) {
  const long long total = (long long)up * K;
  k_resample_taps<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(h, ntaps, up, K, hp);
  return hipGetLastError();
}

hipError_t resample_poly_rows(const ResamplePlan& p, const void* x, int dtype, int channels, const long long* n,
                              long long ldx, int B, int up, int down, const double* hp, double* y, long long ldy,
                              const long long* n_out, hipStream_t s) {
  static const int esize_of[4] = {8, 4, 2, 4};
  const dim3 grid((unsigned)((ldy + p.J - 1) / p.J), (unsigned)B);
  const size_t lds = sizeof(double) * (size_t)p.window;
  if (up == 1)
    k_resample_poly<true><<<grid, RS_THREADS, lds, s>>>(x, dtype, esize_of[dtype], channels, n, ldx, up, down, hp, p.K,
                                                        p.n_pre_remove, p.n_pre_pad, y, ldy, n_out, p.J);
  else
    k_resample_poly<false><<<grid, RS_THREADS, lds, s>>>(x, dtype, esize_of[dtype], channels, n, ldx, up, down, hp, p.K,
                                                         p.n_pre_remove, p.n_pre_pad, y, ldy, n_out, p.J);
  return hipGetLastError();
}

}  // namespace rvcx
