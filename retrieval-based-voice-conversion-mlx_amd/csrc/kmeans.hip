// k-means for building a FAISS IndexIVFFlat on device: nearest-centroid assignment, a stable counting sort of
// the rows by list, the centroid update and the pack into the IvfIndex layout (runtime.h).
//
// Reference call site: rvc/train/process/extract_index.py:58-68 (index_factory(768, "IVF{n},Flat"), train, add),
// which runs faiss-cpu's Clustering::train (Lloyd iterations over IndexFlatL2::search) and IndexIVF::add. The
// driver loop is index_build.cpp.
//
// k_kmeans_assign: assign[q] = argmin_l |x_q - c_l|^2 (ties: lowest l) as argmin_l of the score
// s = |c_l|^2 - 2 x_q . c_l. The dot products run on the exact fp32-input MFMA (v_mfma_f32_32x32x2_f32, as
// conv_gemm.hip's fp32 path): a workgroup owns KM_BQ queries and sweeps the centroids in tiles of KM_BC; the MFMA's
// A operand is the centroid tile and B the query tile, so a lane's 16 accumulators of one 32x32 product are 16
// centroids of ONE query (C/D map: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)). The running
// (min, argmin) is therefore one pair per lane and query sub-tile, kept in registers over the whole sweep; the
// two lane halves and the two centroid-side waves are reduced through LDS once at the end. Nothing of the
// [n][nlist] score matrix is ever stored. Both lane halves take 16 contiguous k of a 32-wide chunk (k = 16 h + j:
// the same permutation of the summation order on both operands), so a fragment is four 16-byte LDS reads.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "device_util.h"
#include "ivf_kernels.h"

namespace rvcx {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KM_BQ = 128;     // queries per workgroup
constexpr int KM_BC = 128;     // centroids per tile
constexpr int KM_CK = 32;      // k per staged chunk
constexpr int KM_LD = KM_CK + 4;  // LDS row stride in floats (16-byte aligned rows, 16-byte reads conflict-free)
constexpr int KM_THREADS = 256;

// (score, id) lexicographic "a strictly before b"
__device__ __forceinline__ bool score_lt(float sa, int ia, float sb, int ib) {
  return sa < sb || (sa == sb && ia < ib);
}

}  // namespace

// ------------------------------------------------------------------ row norms
// norms[r] = sum_i x[r][i]^2, one wave per row, accumulated in fp64 and rounded once
__global__ void __launch_bounds__(256) k_kmeans_norms(const float* __restrict__ x, int rows, int d,
                                                      float* __restrict__ norms) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* p = x + (long long)r * d;
  double acc = 0.0;
  for (int i = lane; i < d; i += 64) {
    const double v = p[i];
    acc += v * v;
  }
  acc = wave_sum(acc);
  if (lane == 0) norms[r] = (float)acc;
}

// ------------------------------------------------------------------ fused distance GEMM + argmin
// grid.x = ceil(n / KM_BQ); 4 waves as 2 (centroid side) x 2 (query side), each 64 centroids x 64 queries per tile
__global__ void __launch_bounds__(KM_THREADS) k_kmeans_assign(const float* __restrict__ x, int n, int d,
                                                             const float* __restrict__ cent,
                                                             const float* __restrict__ cnorm, int nlist,
                                                             int* __restrict__ assign) {
  __shared__ __attribute__((aligned(16))) float cs[KM_BC * KM_LD];  // centroid tile [c][k]
  __shared__ __attribute__((aligned(16))) float xs[KM_BQ * KM_LD];  // query tile [q][k]
  __shared__ float ns[KM_BC];                                       // |c|^2 of the tile, +inf past nlist
  __shared__ float red_s[4][KM_BQ];                                 // end reduction: [centroid wave x lane half][q]
  __shared__ int red_i[4][KM_BQ];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wc = w >> 1, wq = w & 1;
  const int r31 = lane & 31, h = lane >> 5;
  const long long q0 = (long long)blockIdx.x * KM_BQ;

  // staging: thread -> rows (tid >> 3) + 32 i, float4 column (tid & 7)
  const int srow = tid >> 3, scol = (tid & 7) * 4;
  f32x4 xr[4], cr[4];
  auto load_x = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long q = q0 + srow + 32 * i;
      xr[i] = q < n ? *reinterpret_cast<const f32x4*>(x + q * d + k0 + scol) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto load_c = [&](int c0, int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + srow + 32 * i;
      cr[i] = c < nlist ? *reinterpret_cast<const f32x4*>(cent + (long long)c * d + k0 + scol)
                        : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto store_tiles = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<f32x4*>(&xs[(srow + 32 * i) * KM_LD + scol]) = xr[i];
      *reinterpret_cast<f32x4*>(&cs[(srow + 32 * i) * KM_LD + scol]) = cr[i];
    }
  };

  float best[2] = {INFINITY, INFINITY};
  int bidx[2] = {0, 0};  // always a valid list, whatever the data (NaN scores never win)
  const int nchunks = d / KM_CK;

  for (int c0 = 0; c0 < nlist; c0 += KM_BC) {
    f32x16 acc[2][2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;
    __syncthreads();  // the previous tile's score pass has read ns
    if (tid < KM_BC) ns[tid] = c0 + tid < nlist ? cnorm[c0 + tid] : INFINITY;
    load_x(0);
    load_c(c0, 0);
    for (int ch = 0; ch < nchunks; ++ch) {
      __syncthreads();  // the previous chunk's fragment reads (and the previous tile's ns reads) are done
      store_tiles();
      __syncthreads();
      if (ch + 1 < nchunks) {  // the next chunk's global reads fly under this chunk's MFMAs
        load_x((ch + 1) * KM_CK);
        load_c(c0, (ch + 1) * KM_CK);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4 av[2], bv[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          av[t] = *reinterpret_cast<const f32x4*>(&cs[(wc * 64 + t * 32 + r31) * KM_LD + h * 16 + j * 4]);
          bv[t] = *reinterpret_cast<const f32x4*>(&xs[(wq * 64 + t * 32 + r31) * KM_LD + h * 16 + j * 4]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
              acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm][e], bv[tn][e], acc[tm][tn], 0, 0, 0);
      }
    }
    // the tile's scores against the running minimum. A lane meets its centroids in ascending order (tiles, then
    // tm, then r), so strict less keeps the lowest id among equal scores.
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cl = wc * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float nn = ns[cl];  // +inf for a padded centroid: its score is +inf, never 0
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const float s = fmaf(-2.f, acc[tm][tn][r], nn);
          if (s < best[tn]) {
            best[tn] = s;
            bidx[tn] = c0 + cl;
          }
        }
      }
  }
  // reduce the 2 centroid-side waves x 2 lane halves of every query
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    red_s[wc * 2 + h][wq * 64 + tn * 32 + r31] = best[tn];
    red_i[wc * 2 + h][wq * 64 + tn * 32 + r31] = bidx[tn];
  }
  __syncthreads();
  if (tid < KM_BQ && q0 + tid < n) {  // padded query rows are not stored
    float s = red_s[0][tid];
    int i = red_i[0][tid];
#pragma unroll
    for (int p = 1; p < 4; ++p)
      if (score_lt(red_s[p][tid], red_i[p][tid], s, i)) {
        s = red_s[p][tid];
        i = red_i[p][tid];
      }
    assign[q0 + tid] = i;
  }
}

// dist[q] = sum_i (x[q][i] - cent[assign[q]][i])^2 of the chosen centroid (direct form: no cancellation)
__global__ void __launch_bounds__(256) k_kmeans_dist(const float* __restrict__ x, int n, int d,
                                                     const float* __restrict__ cent, const int* __restrict__ assign,
                                                     float* __restrict__ dist) {
  const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n) return;
  const int lane = threadIdx.x & 63;
  const float* xp = x + q * d;
  const float* cp = cent + (long long)assign[q] * d;
  float acc = 0.f;
  for (int i = lane; i < d; i += 64) {
    const float t = xp[i] - cp[i];
    acc = fmaf(t, t, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) dist[q] = acc;
}

// ------------------------------------------------------------------ stable counting sort of the rows by list
// Block b owns the contiguous rows [b rpb, (b + 1) rpb). hist[b][l] counts its rows of list l (integer adds: the
// counts do not depend on their order); the scan turns column l into the block's first rank inside list l and the
// totals into sizes / off; the scatter then walks each block's rows in order, KM_SEG at a time, ranking a row among
// the earlier rows of its segment by comparison. perm therefore holds each list's rows ascending by id, whatever the
// scheduling: no ordering depends on an atomic.
constexpr int KM_SEG = 256;

__global__ void __launch_bounds__(KM_SEG) k_kmeans_hist(const int* __restrict__ assign, int n, int rpb, int nlist,
                                                        int* __restrict__ hist) {
  const long long r0 = (long long)blockIdx.x * rpb;
  const long long r1 = r0 + rpb < n ? r0 + rpb : n;
  int* hb = hist + (long long)blockIdx.x * nlist;
  for (long long r = r0 + threadIdx.x; r < r1; r += KM_SEG) {
    const int key = assign[r];
    if ((unsigned)key < (unsigned)nlist) atomicAdd(&hb[key], 1);  // a row of no list is left out of every list
  }
}

// one thread per list: hist[b][l] <- rows of list l in blocks before b; sizes[l] <- the total
__global__ void __launch_bounds__(256) k_kmeans_scan_blocks(int* __restrict__ hist, int nb, int nlist,
                                                            long long* __restrict__ sizes) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= nlist) return;
  int run = 0;
  for (int b = 0; b < nb; ++b) {
    const int v = hist[(long long)b * nlist + l];
    hist[(long long)b * nlist + l] = run;
    run += v;
  }
  sizes[l] = run;
}

// off[0] = 0, off[l + 1] = off[l] + sizes[l]: one block, 1024 lists per step
__global__ void __launch_bounds__(1024) k_kmeans_scan_lists(const long long* __restrict__ sizes, int nlist,
                                                            long long* __restrict__ off) {
  __shared__ long long sh[1024];
  __shared__ long long carry;
  if (threadIdx.x == 0) {
    carry = 0;
    off[0] = 0;
  }
  __syncthreads();
  for (int base = 0; base < nlist; base += 1024) {
    const int l = base + threadIdx.x;
    sh[threadIdx.x] = l < nlist ? sizes[l] : 0;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const long long v = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
      __syncthreads();
      sh[threadIdx.x] += v;
      __syncthreads();
    }
    if (l < nlist) off[l + 1] = carry + sh[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 1023) carry += sh[1023];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(KM_SEG) k_kmeans_scatter(const int* __restrict__ assign, int n, int rpb, int nlist,
                                                           int* __restrict__ hist, const long long* __restrict__ off,
                                                           int* __restrict__ perm) {
  __shared__ int keys[KM_SEG];
  const long long r0 = (long long)blockIdx.x * rpb;
  const long long r1 = r0 + rpb < n ? r0 + rpb : n;
  int* hb = hist + (long long)blockIdx.x * nlist;  // running first rank of this block inside each list
  const int t = threadIdx.x;
  for (long long s0 = r0; s0 < r1; s0 += KM_SEG) {
    const long long r = s0 + t;
    int key = r < r1 ? assign[r] : -1;
    if ((unsigned)key >= (unsigned)nlist) key = -1;  // as k_kmeans_hist: not counted, not placed
    keys[t] = key;
    __syncthreads();
    int before = 0, base = 0;
    bool last = true;
    if (key >= 0) {
      for (int j = 0; j < t; ++j) before += keys[j] == key ? 1 : 0;
      for (int j = t + 1; j < KM_SEG; ++j) last = last && keys[j] != key;
      base = hb[key];
      perm[off[key] + base + before] = (int)r;
    }
    __syncthreads();  // every row of the segment has read its base
    if (key >= 0 && last) hb[key] = base + before + 1;
    __syncthreads();
  }
}

// ------------------------------------------------------------------ centroid update
// cent[l] = mean of x[perm[off[l] .. off[l + 1])], one block per list, a thread per column, the members added in
// perm order (ascending row id) in fp64 and rounded once. An empty list keeps its centroid.
__global__ void __launch_bounds__(256) k_kmeans_update(const float* __restrict__ x, int d,
                                                       const int* __restrict__ perm, const long long* __restrict__ off,
                                                       float* __restrict__ cent) {
  const int l = blockIdx.x;
  const long long a = off[l], b = off[l + 1];
  if (a == b) return;
  const double cnt = (double)(b - a);
  for (int c = threadIdx.x; c < d; c += 256) {
    double acc = 0.0;
    long long j = a;
    for (; j + 4 <= b; j += 4) {  // four loads in flight, added in order
      const float v0 = x[(long long)perm[j] * d + c], v1 = x[(long long)perm[j + 1] * d + c];
      const float v2 = x[(long long)perm[j + 2] * d + c], v3 = x[(long long)perm[j + 3] * d + c];
      acc += v0;
      acc += v1;
      acc += v2;
      acc += v3;
    }
    for (; j < b; ++j) acc += x[(long long)perm[j] * d + c];
    cent[(long long)l * d + c] = (float)(acc / cnt);
  }
}

// faiss Clustering split_clusters on one (empty list i, donor list j) pair: c_i = c_j, then component k of c_i is
// scaled by 1 + eps (even k) / 1 - eps (odd k) and that of c_j by the opposite
__global__ void __launch_bounds__(256) k_kmeans_split(float* __restrict__ cent, int d, int i, int j, float eps) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= d) return;
  const float v = cent[(long long)j * d + k];
  const float up = 1.f + eps, dn = 1.f - eps;
  cent[(long long)i * d + k] = v * ((k & 1) ? dn : up);
  cent[(long long)j * d + k] = v * ((k & 1) ? up : dn);
}

// ------------------------------------------------------------------ pack into the IvfIndex layout
// vecs[slot] = x[perm[slot]], ids[slot] = perm[slot], slot_of_id[perm[slot]] = slot; one wave per slot
__global__ void __launch_bounds__(256) k_kmeans_pack(const float* __restrict__ x, int n, int d,
                                                     const int* __restrict__ perm, float* __restrict__ vecs,
                                                     long long* __restrict__ ids, int* __restrict__ slot_of_id) {
  const long long slot = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= n) return;
  const int lane = threadIdx.x & 63;
  const int id = perm[slot];
  const float* src = x + (long long)id * d;
  float* dst = vecs + slot * d;
  for (int i = lane; i < d; i += 64) dst[i] = src[i];
  if (lane == 0) {
    ids[slot] = id;
    slot_of_id[id] = (int)slot;
  }
}

// ------------------------------------------------------------------ launchers
bool kmeans_shape_ok(int d) { return d > 0 && d % 32 == 0 && d <= 1024; }

hipError_t kmeans_assign(const float* x, long long n, int d, const float* cent, long long nlist, float* cnorm,
                         int* assign, float* dist, hipStream_t s) {
  if (!kmeans_shape_ok(d) || n <= 0 || nlist <= 0 || n > INT_MAX || nlist > INT_MAX) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(cent)) & 15) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_kmeans_norms, dim3((unsigned)((nlist + 3) / 4)), dim3(256), 0, s, cent, (int)nlist, d, cnorm);
  hipLaunchKernelGGL(k_kmeans_assign, dim3((unsigned)((n + KM_BQ - 1) / KM_BQ)), dim3(KM_THREADS), 0, s, x, (int)n, d,
                     cent, cnorm, (int)nlist, assign);
  if (dist)
    hipLaunchKernelGGL(k_kmeans_dist, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, x, (int)n, d, cent, assign,
                       dist);
  return hipGetLastError();
}

int kmeans_sort_blocks(long long n) {
  const long long nb = (n + 4 * KM_SEG - 1) / (4 * KM_SEG);
  return (int)(nb < 1 ? 1 : nb > 256 ? 256 : nb);
}

hipError_t kmeans_sort(const int* assign, long long n, long long nlist, int* hist, long long* sizes, long long* off,
                       int* perm, hipStream_t s) {
  if (n <= 0 || nlist <= 0 || n > INT_MAX || nlist > INT_MAX) return hipErrorInvalidValue;
  const int nb = kmeans_sort_blocks(n);
  const int rpb = (int)((n + nb - 1) / nb);
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)nb * nlist * sizeof(int), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_kmeans_hist, dim3(nb), dim3(KM_SEG), 0, s, assign, (int)n, rpb, (int)nlist, hist);
  hipLaunchKernelGGL(k_kmeans_scan_blocks, dim3((unsigned)((nlist + 255) / 256)), dim3(256), 0, s, hist, nb,
                     (int)nlist, sizes);
  hipLaunchKernelGGL(k_kmeans_scan_lists, dim3(1), dim3(1024), 0, s, sizes, (int)nlist, off);
  hipLaunchKernelGGL(k_kmeans_scatter, dim3(nb), dim3(KM_SEG), 0, s, assign, (int)n, rpb, (int)nlist, hist, off,
                     perm);
  return hipGetLastError();
}

hipError_t kmeans_update(const float* x, int d, const int* perm, const long long* off, long long nlist, float* cent,
                         hipStream_t s) {
  hipLaunchKernelGGL(k_kmeans_update, dim3((unsigned)nlist), dim3(256), 0, s, x, d, perm, off, cent);
  return hipGetLastError();
}

hipError_t kmeans_split(float* cent, int d, long long i, long long j, float eps, hipStream_t s) {
  hipLaunchKernelGGL(k_kmeans_split, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, cent, d, (int)i, (int)j, eps);
  return hipGetLastError();
}

hipError_t kmeans_pack(const float* x, long long n, int d, const int* perm, float* vecs, long long* ids,
                       int* slot_of_id, hipStream_t s) {
  hipLaunchKernelGGL(k_kmeans_pack, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, x, (int)n, d, perm, vecs, ids,
                     slot_of_id);
  return hipGetLastError();
}

}  // namespace rvcx
