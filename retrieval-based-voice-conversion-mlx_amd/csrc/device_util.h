// Device helpers shared by the non-GEMM kernel files: the elementwise launch geometry, the 64-lane butterfly
// reductions and the counter-based random draws. One definition each; a file that needs one includes this.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rvcx {

namespace {

constexpr int TB = 256;

inline unsigned nblocks(long long n, int per = TB) {
  long long b = (n + per - 1) / per;
  if (b > 65535LL * 32) b = 65535LL * 32;
  return (unsigned)(b < 1 ? 1 : b);
}

// xor butterfly over the 64 lanes of a wave in the order 32, 16, ..., 1: every lane ends with the result
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- Philox4x32-10 (counter-based; one 128-bit block per 4 normals)
__device__ __forceinline__ void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
// Draw idx of the stream (seed, domain0, domain1): the two domain words fill the counter's upper half, so the draws of
// two call sites with different domains never share a Philox block. normal_at: Box-Muller, two normals per block.
__device__ __forceinline__ float normal_at(uint64_t seed, uint64_t idx, uint32_t domain0, uint32_t domain1) {
  uint32_t c[4] = {(uint32_t)(idx >> 1), (uint32_t)(idx >> 33), domain0, domain1};
  philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const float u1 = ((c[0] >> 8) + 1) * (1.0f / 16777217.0f);
  const float u2 = (c[1] >> 8) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.f * logf(u1));
  const float th = 6.283185307179586f * u2;
  return (idx & 1) ? r * sinf(th) : r * cosf(th);
}
__device__ __forceinline__ float uniform_at(uint64_t seed, uint64_t idx, uint32_t domain0, uint32_t domain1) {
  uint32_t c[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), domain0, domain1};
  philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return (c[0] >> 8) * (1.0f / 16777216.0f);  // [0, 1)
}

}  // namespace

}  // namespace rvcx
