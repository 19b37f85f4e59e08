// rvcx kernel launchers (internal; the public C-ABI is include/rvcx.h): what every launcher header shares.
//
// Tensor convention on device: frame-major ("time-major") rows, channels
// contiguous: a [T][C] matrix with row stride ld (floats). 2-D images (RMVPE
// U-Net) are NHWC: pixel-major rows (h*W + w), channels contiguous.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rvcx {

// Process-wide developer knobs (RVCX_* environment variables: A/B switches, tile / split-K policy overrides, the
// contraction arithmetic): honoured ONLY when RVCX_EXPERIMENTAL=1 is set, so a stray variable in a user's shell cannot
// change a result or a kernel path. Returns getenv(name), or nullptr without the opt-in. rvcx_config_info reports
// the opt-in and every RVCX_* variable present (honoured or ignored). Defined in capi.cpp.
const char* rvcx_knob(const char* name);

// A length per row of a batch: one value for every row, or a device array indexed by the row (read on the device only)
struct Len {
  const int* v = nullptr;
  int n = 0;
  Len(int all) : n(all) {}
  Len(const int* rows) : v(rows) {}
  __host__ __device__ int operator[](int b) const { return v ? v[b] : n; }
};

enum Act : int {
  ACT_NONE = 0,
  ACT_LRELU = 1,    // leaky relu with slope
  ACT_RELU = 2,
  ACT_GELU = 3,     // exact erf GELU (HF "gelu", torch F.gelu default)
  ACT_TANH = 4,
  ACT_SIGMOID = 5,
  ACT_LOGCLAMP = 6, // log(max(v, slope))  (RMVPE mel: log(clamp(.,1e-5)))
};

}  // namespace rvcx
