// Pipeline.get_f0's adjustments of the f0 track on device, fp64 like numpy: the shift and the coarse (mel) quantisation
// with a correctly rounded log (dd_math.h), and autotune's snap to the nearest note.
#include <cmath>

#include "dd_math.h"
#include "device_util.h"
#include "pipeline_kernels.h"

// a product and a sum fuse within one expression only, never across statements (the kernels below switch it off)
#pragma clang fp contract(on)

namespace rvcx {

// ------------------------------------------------------------------ f0 shift + coarse quantisation (pipeline.py:280-291)
__global__ void k_f0post(const double* f0, int F, double shift, int32_t* coarse, float* pitchf, double* f0_out) {
#pragma clang fp contract(off)  // numpy rounds every product and sum separately
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F) return;
  const double f = f0[i] * shift;
  // self.f0_mel_min / f0_mel_max = 1127 * np.log(1 + 50/700), 1127 * np.log(1 + 1100/700) (pipeline.py:195-196):
  // numpy, glibc and the correctly rounded log agree on both
  constexpr double mel_min = 0x1.370515d9beb10p+6;
  constexpr double mel_max = 0x1.0a1a207dfdbe5p+10;
  // log correctly rounded (dd_math.h): the coarse pitch is integer output; every other step is one IEEE op
  double m = 1127.0 * dd::log_cr(1.0 + f / 700.0);
  if (m > 0) m = (m - mel_min) * 254.0 / (mel_max - mel_min) + 1.0;
  if (m <= 1) m = 1;
  if (m > 255) m = 255;
  coarse[i] = (int32_t)rint(m);
  pitchf[i] = (float)f;
  if (f0_out) f0_out[i] = f;
}
hipError_t f0_post(const double* f0, int F, double shift, int32_t* coarse, float* pitchf, double* f0_out,
                   hipStream_t s) {
  hipLaunchKernelGGL(k_f0post, dim3(nblocks(F)), dim3(TB), 0, s, f0, F, shift, coarse, pitchf, f0_out);
  return hipGetLastError();
}

// ------------------------------------------------------------------ get_f0 adjustments
// Autotune.autotune_f0 (rvc/infer/pipeline.py:151-162): snap to the nearest of 54 note
// frequencies (first minimum wins, like Python's min()), blend by strength. The rvc/ path snaps
// every frame (f0 = 0 -> 49 Hz * strength); rvc_mlx (pipeline_mlx.py:72-80) leaves f0 <= 0 alone.
__constant__ double c_notes[54] = {
    49.00,  51.91,  55.00,  58.27,  61.74,  65.41,  69.30,  73.42,  77.78,  82.41,  87.31,  92.50,  98.00,  103.83,
    110.00, 116.54, 123.47, 130.81, 138.59, 146.83, 155.56, 164.81, 174.61, 185.00, 196.00, 207.65, 220.00, 233.08,
    246.94, 261.63, 277.18, 293.66, 311.13, 329.63, 349.23, 369.99, 392.00, 415.30, 440.00, 466.16, 493.88, 523.25,
    554.37, 587.33, 622.25, 659.25, 698.46, 739.99, 783.99, 830.61, 880.00, 932.33, 987.77, 1046.50};

__global__ void k_autotune(double* f0, int F, double strength, int skip_unvoiced) {
#pragma clang fp contract(off)  // numpy rounds every product and sum separately
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F) return;
  const double f = f0[i];
  if (skip_unvoiced && f <= 0.0) return;
  double best = c_notes[0], bd = fabs(c_notes[0] - f);
  for (int j = 1; j < 54; ++j) {
    const double d = fabs(c_notes[j] - f);
    if (d < bd) {
      bd = d;
      best = c_notes[j];
    }
  }
  f0[i] = f + (best - f) * strength;
}
hipError_t f0_autotune(double* f0, int F, double strength, int skip_unvoiced, hipStream_t s) {
  hipLaunchKernelGGL(k_autotune, dim3(nblocks(F)), dim3(TB), 0, s, f0, F, strength, skip_unvoiced);
  return hipGetLastError();
}
// The same per row of f0 [B][F] (blockIdx.y = row) with each row's own strength; rows with on[b] == 0 are not touched.
__global__ void k_autotune_rows(double* f0, int F, const double* __restrict__ strength, const int* __restrict__ on) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F || !on[b]) return;
  double* row = f0 + (long long)b * F;
  const double f = row[i];
  double best = c_notes[0], bd = fabs(c_notes[0] - f);
  for (int j = 1; j < 54; ++j) {
    const double d = fabs(c_notes[j] - f);
    if (d < bd) {
      bd = d;
      best = c_notes[j];
    }
  }
  row[i] = f + (best - f) * strength[b];
}
hipError_t f0_autotune_rows(double* f0, int F, const double* strength, const int* on, int B, hipStream_t s) {
  if (F <= 0 || B < 1) return hipSuccess;
  hipLaunchKernelGGL(k_autotune_rows, dim3(nblocks(F), B), dim3(TB), 0, s, f0, F, strength, on);
  return hipGetLastError();
}

}  // namespace rvcx
