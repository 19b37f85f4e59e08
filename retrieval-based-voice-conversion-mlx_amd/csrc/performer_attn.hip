// Performer (FAVOR+) linear attention of the FCPE pitch network: SelfAttention / FastAttention / softmax_kernel /
// linear_attention of rvc/lib/predictors/FCPE.py:179-212, :354-363, :399-559 (non-causal, no local heads).
//
// Per head, with x' = c x (c = D^-0.25, D = 64), P [M][D] the random-feature matrix (M = 266), ratio = M^-0.5:
//   dash = x' P^T                      diag = |x|^2 / 2 * c^2
//   q'   = ratio (exp(dash_q - diag_q - rowmax(dash_q)) + 1e-4)
//   k'   = ratio  exp(dash_k - diag_k + 1e-4)                       (no max subtraction on the keys)
//   ctx  = k'^T v [M][D],  ksum = sum_t k' [M],   out = (q' ctx) / (q' . ksum + 1e-8)
//
// Two passes, both on v_mfma_f32_16x16x4_f32 (an exact fp32 fma chain; the network is a few GFLOP per utterance,
// far below what the split-bf16 planes would buy), no LDS, no barriers, no atomics:
//   pass A (k_perf_kv)   one workgroup per (time slab of 128 rows, head, stream); wave w owns the feature tiles w, w + 4, ...
//                        For a 16-row time tile it forms dash [t][j] (D layout: row t = 4 kq + r, column j = li),
//                        turns it into k' in registers and feeds it straight back as the B operand of
//                        ctx^T [d][j] += v^T [d][t] k' [t][j] (the k slot kq of step r is t = 4 kq + r). The slab's
//                        ctx and ksum go to their own partial image; k_perf_combine adds the slabs in slab order, so
//                        the result does not depend on scheduling (run-to-run bit identical).
//   pass B (k_perf_out)  one wave per 16 time rows. dash^T [j][t] (row j = 4 kq + r of tile jt, column t = li) stays
//                        in registers; rowmax and the denominator reduce over the lanes of equal li; q'^T is the B
//                        operand of out^T [d][t] += ctx^T [d][j] q'^T [j][t] as it stands.
// Padding: M is no multiple of 16. The loads of feature columns j >= M are clamped to row M - 1 of P, so a padded
// column holds a copy of column M - 1: it cannot move the row maximum (the index mask there is belt and braces), but
// it would count twice in ksum, ctx and the denominator. Their q' / k' are therefore set to zero by index after the
// exponential (exp(0) + eps is not zero), so they add exactly nothing to ksum, ctx, the denominator or the output.
// Time rows t >= T get k' = 0 (pass A) and are not stored (pass B); their loads are clamped to row T - 1, so every
// operand is finite.
// Batch: B streams of one T per launch (grid z). Everything reduced over time -- ksum, ctx, the query's row maximum,
// the denominator -- belongs to one (stream, head): the workspace holds ctx / ksum and the slabs' images per
// (stream, head), and no load is clamped or reduced across a stream's rows. B = 1 is the single-utterance form.
// Ragged: with Tv (a device array) stream b has Tv[b] <= T rows inside its T-row slot. The length is indexed by
// blockIdx.z, so it is one scalar load and every branch on it is wave-uniform (the MFMAs sit inside them). Pass A ends
// the stream's keys at Tv[b] and clamps its loads to row Tv[b] - 1; a slab wholly past Tv[b] loads nothing and writes
// its zero image, so k_perf_combine adds the same slabs for every stream, the extra ones exact zeros: ctx / ksum, and
// with them the output rows, are the B = 1 call's on that stream bit for bit. Pass B's waves past Tv[b] exit, rows past
// Tv[b] are not stored.
#include <cmath>

#include "fcpe_kernels.h"

namespace rvcx {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PD = 64;         // head dimension
constexpr int PA_SLAB = PERFORMER_SLAB;  // time rows per pass-A workgroup
constexpr int PA_WAVES = 4;
constexpr int PA_MAXJT = PERFORMER_MAX_FEATURES / 16 / PA_WAVES;  // feature tiles per wave
constexpr int PB_MAXJT = PERFORMER_MAX_FEATURES / 16;

struct PerfArgs {
  const float* q;
  const float* k;
  const float* v;  // element (b, h, t, d) at p + b bs + h hs + t ld + d
  long long bs, hs;
  int ld;
  const float* P;  // [M][64]
  int M, T, H;
  const int* Tv;  // rows per stream (device), or null: T
  float c, c2, ratio;
};

__device__ __forceinline__ float xor_sum16(float v) {  // over the 4 lanes of equal (lane & 15)
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// rows t0 + li of x (clamped to T - 1), columns 16 g + 4 kq .. + 3: the operand fragments of x' = c x, and
// diag = |x|^2 / 2 * c^2 of row t0 + li (every lane of that li)
__device__ __forceinline__ float load_rows(const float* X, int ld, int t0, int T, int li, int kq, float c, float c2,
                                           f32x4 (&x)[4]) {
  const int t = min(t0 + li, T - 1);
  float ss = 0.f;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    x[g] = *reinterpret_cast<const f32x4*>(X + (long long)t * ld + 16 * g + 4 * kq);
#pragma unroll
    for (int s = 0; s < 4; ++s) ss += x[g][s] * x[g][s];
    x[g] = x[g] * c;
  }
  return (xor_sum16(ss) * 0.5f) * c2;
}

__global__ __launch_bounds__(256) void k_perf_kv(PerfArgs a, float* part_ctx, float* part_ks) {
  const int slab = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4;
  const int njt = (a.M + 15) / 16;
  const float* K = a.k + b * a.bs + h * a.hs;
  const float* V = a.v + b * a.bs + h * a.hs;
  const int T = a.Tv ? a.Tv[b] : a.T;  // scalar: b is blockIdx.z
  const int t_begin = slab * PA_SLAB, t_end = min(T, t_begin + PA_SLAB);
  f32x4 acc[PA_MAXJT][4];  // ctx^T tile (jj, dt): row d = 16 dt + 4 kq + r, column j = 16 (wave + 4 jj) + li
  float ks[PA_MAXJT];
#pragma unroll
  for (int jj = 0; jj < PA_MAXJT; ++jj) {
    ks[jj] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[jj][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int t0 = t_begin; t0 < t_end; t0 += 16) {
    f32x4 xa[4];
    const float diag_li = load_rows(K, a.ld, t0, T, li, kq, a.c, a.c2, xa);
    float diag[4], va[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      diag[r] = __shfl(diag_li, 4 * kq + r, 64);  // row t0 + 4 kq + r
      const int tv = min(t0 + 4 * kq + r, T - 1);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) va[r][dt] = V[(long long)tv * a.ld + 16 * dt + li];
    }
#pragma unroll
    for (int jj = 0; jj < PA_MAXJT; ++jj) {
      const int jt = wave + PA_WAVES * jj;  // wave-uniform
      if (jt < njt) {
        const int j = 16 * jt + li;
        const float* Pj = a.P + (long long)min(j, a.M - 1) * PD + 4 * kq;
        f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 pb = *reinterpret_cast<const f32x4*>(Pj + 16 * g);
#pragma unroll
          for (int s = 0; s < 4; ++s) d = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[g][s], pb[s], d, 0, 0, 0);
        }
        float kp[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = (t0 + 4 * kq + r < t_end) && (j < a.M);
          kp[r] = ok ? a.ratio * expf(d[r] - diag[r] + 1e-4f) : 0.f;
          ks[jj] += kp[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
            acc[jj][dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[r][dt], kp[r], acc[jj][dt], 0, 0, 0);
      }
    }
  }
  const long long img = ((long long)slab * gridDim.z + b) * a.H + h;  // image (slab, stream, head)
  float* pc = part_ctx + img * a.M * PD;
  float* pk = part_ks + img * a.M;
#pragma unroll
  for (int jj = 0; jj < PA_MAXJT; ++jj) {
    const int jt = wave + PA_WAVES * jj;
    if (jt < njt) {
      const int j = 16 * jt + li;
      const float s = xor_sum16(ks[jj]);
      if (j < a.M) {
        if (kq == 0) pk[j] = s;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4*>(pc + (long long)j * PD + 16 * dt + 4 * kq) = acc[jj][dt];
      }
    }
  }
}

// ctx / ksum = the slabs' partial images added in slab order (n_ctx / n_ks: the elements of all streams and heads)
__global__ void k_perf_combine(const float* part_ctx, const float* part_ks, int nslab, long long n_ctx, long long n_ks,
                               float* ctx, float* ksum) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i < n_ctx) {
    float s = part_ctx[i];
    for (int p = 1; p < nslab; ++p) s += part_ctx[p * n_ctx + i];
    ctx[i] = s;
  } else if (i < n_ctx + n_ks) {
    const long long k = i - n_ctx;
    float s = part_ks[k];
    for (int p = 1; p < nslab; ++p) s += part_ks[p * n_ks + k];
    ksum[k] = s;
  }
}

__global__ __launch_bounds__(256) void k_perf_out(PerfArgs a, const float* ctx, const float* ksum, float* out,
                                                   long long out_bs, long long out_hs, int out_ld) {
  const int h = blockIdx.y, b = blockIdx.z;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4;
  const int t0 = (blockIdx.x * 4 + wave) * 16;
  const int T = a.Tv ? a.Tv[b] : a.T;  // scalar: b is blockIdx.z
  if (t0 >= T) return;
  const int njt = (a.M + 15) / 16;
  f32x4 xb[4];
  const float diag = load_rows(a.q + b * a.bs + h * a.hs, a.ld, t0, T, li, kq, a.c, a.c2, xb);  // row t0 + li
  f32x4 dsh[PB_MAXJT];  // dash^T tile jt: row j = 16 jt + 4 kq + r, column t = t0 + li
  float mx = -INFINITY;
#pragma unroll
  for (int jt = 0; jt < PB_MAXJT; ++jt) {
    if (jt < njt) {
      const float* Pj = a.P + (long long)min(16 * jt + li, a.M - 1) * PD + 4 * kq;
      f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 pa = *reinterpret_cast<const f32x4*>(Pj + 16 * g);
#pragma unroll
        for (int s = 0; s < 4; ++s) d = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[s], xb[g][s], d, 0, 0, 0);
      }
      dsh[jt] = d;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * jt + 4 * kq + r < a.M) mx = fmaxf(mx, d[r]);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float* C = ctx + ((long long)b * a.H + h) * a.M * PD;
  const float* KS = ksum + ((long long)b * a.H + h) * a.M;
  float den = 0.f;
  f32x4 o[4];  // out^T tile dt: row d = 16 dt + 4 kq + r, column t = t0 + li
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int jt = 0; jt < PB_MAXJT; ++jt) {
    if (jt < njt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * jt + 4 * kq + r;
        const int jc = min(j, a.M - 1);
        const float qp = j < a.M ? a.ratio * (expf(dsh[jt][r] - diag - mx) + 1e-4f) : 0.f;
        den += qp * KS[jc];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(C[(long long)jc * PD + 16 * dt + li], qp, o[dt], 0, 0, 0);
      }
    }
  }
  const float dinv = 1.f / (xor_sum16(den) + 1e-8f);
  if (t0 + li < T) {
    float* y = out + b * out_bs + h * out_hs + (long long)(t0 + li) * out_ld + 4 * kq;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4*>(y + 16 * dt) = o[dt] * dinv;
  }
}

}  // namespace

int performer_slabs(int T) { return (T + PA_SLAB - 1) / PA_SLAB; }

long long performer_ws_floats(int H, int T, int M, int B) {
  const int ns = performer_slabs(T);
  const long long one = (long long)B * H * M * (PD + 1);
  return one + (ns > 1 ? ns * one : 0);
}

hipError_t performer_attention(const float* q, const float* k, const float* v, long long hs, int ld, int H, int T,
                               const float* P, int M, float* ws, float* out, long long out_hs, int out_ld,
                               hipStream_t s, int B, long long bs, long long out_bs, const int* Tv) {
  if (H < 1 || T < 1 || M < 1 || M > PERFORMER_MAX_FEATURES || (ld & 3) || (hs & 3) || (out_ld & 3) || (out_hs & 3) ||
      B < 1 || B > 65535 || (bs & 3) || (out_bs & 3))
    return hipErrorInvalidValue;
  for (const void* p : {(const void*)q, (const void*)k, (const void*)v, (const void*)P, (const void*)ws,
                        (const void*)out})
    if (!p || (reinterpret_cast<uintptr_t>(p) & 15)) return hipErrorInvalidValue;
  PerfArgs a;
  a.q = q;
  a.k = k;
  a.v = v;
  a.bs = bs;
  a.hs = hs;
  a.ld = ld;
  a.P = P;
  a.M = M;
  a.T = T;
  a.H = H;
  a.Tv = Tv;
  a.c = 1.f / sqrtf(sqrtf((float)PD));  // 64^-0.25 (FCPE.py:185)
  a.c2 = a.c * a.c;
  a.ratio = (float)(1.0 / std::sqrt((double)M));  // M^-0.5 (FCPE.py:188)
  const int ns = performer_slabs(T);
  const long long n_ctx = (long long)B * H * M * PD, n_ks = (long long)B * H * M;
  // ws: ctx | the slabs' ctx images | ksum | the slabs' ksum images (the ctx images first: they take 16-byte stores)
  float* ctx = ws;
  float* part_ctx = ns > 1 ? ctx + n_ctx : ctx;  // one slab: pass A writes the final images
  float* ksum = ctx + (ns > 1 ? 1 + ns : 1) * n_ctx;
  float* part_ks = ns > 1 ? ksum + n_ks : ksum;
  hipLaunchKernelGGL(k_perf_kv, dim3(ns, H, B), dim3(256), 0, s, a, part_ctx, part_ks);
  if (ns > 1)
    hipLaunchKernelGGL(k_perf_combine, dim3((unsigned)((n_ctx + n_ks + 255) / 256)), dim3(256), 0, s, part_ctx,
                       part_ks, ns, n_ctx, n_ks, ctx, ksum);
  hipLaunchKernelGGL(k_perf_out, dim3((T + 63) / 64, H, B), dim3(256), 0, s, a, ctx, ksum, out, out_bs, out_hs, out_ld);
  return hipGetLastError();
}

}  // namespace rvcx
