// Polyphase resampling on device (resample.hip): scipy.signal.resample_poly with decode and channel downmix fused in
#pragma once
#include "kernel_base.h"

namespace rvcx {

// What a (up, down, ntaps) triple fixes, with half = (ntaps - 1) / 2 (scipy.signal.resample_poly's own quantities):
// K = ceil(ntaps / up) taps per output, n_pre_pad = down - half % down, n_pre_remove = (half + n_pre_pad) / down.
// J outputs per block and the block's staged window in doubles; J == 0: K alone exceeds the window a block can stage
struct ResamplePlan {
  int K = 0, J = 0, window = 0;
  long long n_pre_pad = 0, n_pre_remove = 0;
};
ResamplePlan resample_poly_plan(int up, int down, long long ntaps);

// h [ntaps] -> hp [up][K] phase-major, zero-filled
hipError_t resample_poly_taps(const double* h, long long ntaps, int up, int K, double* hp, hipStream_t s);

// Row b: n[b] frames of `channels` interleaved samples of dtype (0 f64, 1 f32, 2 i16 * 2^-15, 3 i32 * 2^-31) at
// x + b*ldx frames -> y[b][0 .. n_out[b]) = resample_poly(mean over channels, up, down); y[b][n_out[b] .. ldy) = 0.
// n, n_out: device arrays. fp64 fma in ascending input order; a row's result does not depend on B.
hipError_t resample_poly_rows(const ResamplePlan& p, const void* x, int dtype, int channels, const long long* n,
                              long long ldx, int B, int up, int down, const double* hp, double* y, long long ldy,
                              const long long* n_out, hipStream_t s);

}  // namespace rvcx
