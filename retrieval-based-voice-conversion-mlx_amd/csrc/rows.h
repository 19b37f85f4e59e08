// What every "rows of different lengths" form is built from (the _v forwards, pipeline_forward_rows, their C entries):
// the rows' description, the staging of strided outputs, the per-row lengths the kernels read on device. Host code.
#pragma once
#include <algorithm>

#include "runtime.h"

namespace rvcx {

// B rows of nv[b] samples (host array), or of n samples each, at stride ld. Refused as RVCX_E_INVALID with the caller's
// prefix: no rows, a stride shorter than the longest of several rows, a row below lo samples (the C entries' 1).
struct Rows {
  int B;
  int64_t n_max, n_min;
  bool equal;
  Rows(const std::string& who, int64_t n, int B_, int64_t ld) : B(B_), n_max(n), n_min(n), equal(true) {
    if (B < 1) throw Error(RVCX_E_INVALID, who + ": batch < 1");
    if (ld < n_max && B > 1) throw Error(RVCX_E_INVALID, who + ": row stride shorter than the longest row");
  }
  Rows(const std::string& who, const int64_t* nv, int B_, int64_t ld, int64_t lo = INT64_MIN)
      : Rows(who, B_ < 1 ? 0 : *std::max_element(nv, nv + B_), B_, ld) {
    n_min = *std::min_element(nv, nv + B);
    equal = n_min == n_max;
    if (n_min < lo) throw Error(RVCX_E_INVALID, who + ": bad row length");
  }
};

// An output of B rows that a pass writes `tight` elements apart for a caller whose rows lie `ld` apart: p, where it
// writes, is the caller's pointer when the two agree, one row or no output, else pool buffer `name` till copy_out().
template <class T>
struct Staged {
  T *user, *p;
  size_t ld, tight, B;
  Staged(Ctx& c, const char* name, T* user_, int64_t ld_, int64_t tight_, int B_, hipStream_t s)
      : user(user_), p(user_), ld((size_t)ld_), tight((size_t)tight_), B((size_t)B_) {
    if (user && ld != tight && B > 1) p = c.buf<T>(name, B * tight, s);
  }
  void copy_out(hipStream_t s) const {
    if (p != user)
      RVCX_HIP(hipMemcpy2DAsync(user, ld * sizeof(T), p, tight * sizeof(T), tight * sizeof(T), B,
                                hipMemcpyDeviceToDevice, s));
  }
};

// Per-row int32 lengths for the kernels: ncol columns of B values, filled on the host through at(), then uploaded into
// the pool buffer `name` with one copy; col(k) is column k on device.
struct LenCols {
  std::vector<int32_t> h;
  int B;
  int32_t* d = nullptr;
  LenCols(int ncol, int B_) : h((size_t)ncol * B_), B(B_) {}
  int32_t& at(int k, int b) { return h[(size_t)k * B + b]; }
  const int32_t* col(int k) const { return d + (size_t)k * B; }
  void upload(Ctx& c, const char* name, hipStream_t s) {
    d = c.buf<int32_t>(name, h.size(), s);
    RVCX_HIP(hipMemcpyAsync(d, h.data(), sizeof(int32_t) * h.size(), hipMemcpyHostToDevice, s));
  }
};

}  // namespace rvcx
