// The retrieval index on device: IndexIVFFlat search and blend (ivf.hip) and the k-means that builds it (kmeans.hip)
#pragma once
#include "kernel_base.h"

namespace rvcx {

// FAISS IndexIVFFlat on device (ivf.hip): search + the retrieval blend of pipeline.py:378-388
struct IvfView {
  int d = 0, nprobe = 1;
  long long nlist = 0, ntotal = 0;
  const float* cent = nullptr;       // [nlist][d]
  const float* vecs = nullptr;       // [ntotal][d], list order
  const long long* off = nullptr;    // [nlist + 1]
  const long long* ids = nullptr;    // [ntotal], list order
  const int* slot_of_id = nullptr;   // [ntotal]
};
constexpr int IVF_MAX_K = 16;
size_t ivf_ws_floats(long long n, long long nlist, int nprobe);
// dist_out/ids_out [n][k] (optional); out [n][d] = retrieval blend (optional)
hipError_t ivf_search(const IvfView& v, const float* x, long long n, int k, float* dist_out, long long* ids_out,
                      float rate, float one_minus_rate, float* out, float* ws, hipStream_t s);
// The retrieval blend for a chosen set of sequences of a batch x / out [B][L][d] in one search: query q is row
// off + q % (L - off) of sequence seqs[q / (L - off)], blended at that sequence's own rate[seq] / one_minus_rate[seq]
// (device arrays indexed by sequence). Rows that are no query are not written. n_seq * (L - off) queries.
struct IvfRows {
  const int* seqs = nullptr;  // null: query q is row q of x / out (ivf_search)
  const float* rate = nullptr;
  const float* one_minus_rate = nullptr;
  int L = 0, off = 0;
};
hipError_t ivf_retrieve_rows(const IvfView& v, const float* x, const IvfRows& rows, int n_seq, float* out, float* ws,
                             hipStream_t s);

// k-means for building an IndexIVFFlat (kmeans.hip; the Lloyd loop is index_build.cpp). x [n][d], cent [nlist][d]
// fp32 row-major, 16-byte aligned; d % 32 == 0 and d <= 1024 (kmeans_shape_ok), n and nlist below 2^31.
bool kmeans_shape_ok(int d);
// assign[q] = argmin_l |x_q - c_l|^2, ties to the lowest l (fp32-input MFMA, no [n][nlist] store); dist [n]
// (optional) = the squared distance to that centroid. cnorm [nlist] is scratch for the centroid norms.
hipError_t kmeans_assign(const float* x, long long n, int d, const float* cent, long long nlist, float* cnorm,
                         int* assign, float* dist, hipStream_t s);
// Stable counting sort of the rows by list: sizes [nlist], off [nlist + 1], perm [n] = row ids grouped by list,
// ascending inside each list (the order faiss's add fills a list in); identical run to run. hist is scratch of
// kmeans_sort_blocks(n) * nlist ints. A row whose assign is outside [0, nlist) is left out of every list.
int kmeans_sort_blocks(long long n);
hipError_t kmeans_sort(const int* assign, long long n, long long nlist, int* hist, long long* sizes, long long* off,
                       int* perm, hipStream_t s);
// cent[l] <- the mean of its members (fp64 accumulation in perm order, one rounding); an empty list keeps its own
hipError_t kmeans_update(const float* x, int d, const int* perm, const long long* off, long long nlist, float* cent,
                         hipStream_t s);
// faiss split_clusters for one pair: c_i = c_j scaled by 1 +- eps on even / odd components, c_j by the opposite
hipError_t kmeans_split(float* cent, int d, long long i, long long j, float eps, hipStream_t s);
// the IvfView arrays from perm: vecs [n][d] in list order, ids [n], slot_of_id [n]
hipError_t kmeans_pack(const float* x, long long n, int d, const int* perm, float* vecs, long long* ids,
                       int* slot_of_id, hipStream_t s);

}  // namespace rvcx
