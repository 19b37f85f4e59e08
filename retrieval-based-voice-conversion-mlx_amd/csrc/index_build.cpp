// Building and writing a FAISS IndexIVFFlat on device.
//
// Replaces faiss.index_factory(768, f"IVF{n_ivf},Flat") + train + add + faiss.write_index of
// rvc/train/process/extract_index.py:58-70. index_build restates faiss 1.7.4 Clustering::train (Lloyd iterations
// over an IndexFlatL2 assignment, cp.niter = 10 for the IVF coarse quantizer) and IndexIVF::add (sequential ids,
// each vector appended to the list of its nearest centroid) on the kernels of kmeans.hip.
//
// Parity status: UNPINNED against faiss itself, as all of the index path is (no faiss and no .index fixture exist
// beside the reference); anchored on faiss's published algorithm and on the fp64 oracle's Lloyd trajectory. Known
// deviations from faiss:
//   * initial centroids: faiss draws them with its own RandomGenerator permutation; here they are the caller's rows
//     (init_rows) or a PCG32 partial shuffle of `seed`.
//   * empty lists: faiss's split_clusters picks the donor at random with probability ~ (size - 1); here the donor
//     is the currently largest list (lowest id among equals), so a build is reproducible. The perturbation
//     (1 +- 1/1024 on even / odd components) and the size bookkeeping are faiss's.
//   * no training subsample: faiss caps training at 256 points per centroid, which with the reference's
//     n_ivf = min(16 sqrt(N), N // 39) needs N > 16.7 M rows to trigger; it is not built.
// Distances are fp32 (exact-f32 MFMA dot products; faiss uses fp32 BLAS/SIMD of its own summation order).
#include <algorithm>
#include <cstring>
#include <unordered_map>

#include "runtime.h"

namespace rvcx {

namespace {

void dev_alloc(DevBuf& b, size_t bytes) {
  bytes = std::max<size_t>(bytes, 16);
  if (hipMalloc(&b.p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    throw Error(RVCX_E_OOM, "index_build: device allocation of " + std::to_string(bytes) + " B failed");
  }
  b.bytes = bytes;
}

// PCG32 (XSH-RR 64/32, O'Neill 2014)
struct Pcg32 {
  uint64_t state, inc;
  explicit Pcg32(uint64_t seed) : state(0), inc((0xda3e39cb94b95bdbULL << 1) | 1) {
    next();
    state += seed;
    next();
  }
  uint32_t next() {
    const uint64_t old = state;
    state = old * 6364136223846793005ULL + inc;
    const uint32_t xs = (uint32_t)(((old >> 18) ^ old) >> 27), rot = (uint32_t)(old >> 59);
    return (xs >> rot) | (xs << ((32 - rot) & 31));
  }
  uint32_t below(uint32_t bound) {  // unbiased
    const uint32_t thresh = (0u - bound) % bound;
    for (;;) {
      const uint32_t r = next();
      if (r >= thresh) return r % bound;
    }
  }
};

// the first nlist entries of a seeded Fisher-Yates shuffle of 0..n-1 (sparse: only the touched entries are kept)
std::vector<int32_t> seeded_rows(int64_t n, int64_t nlist, uint64_t seed) {
  Pcg32 rng(seed);
  std::unordered_map<int64_t, int64_t> moved;
  auto at = [&](int64_t i) {
    auto it = moved.find(i);
    return it == moved.end() ? i : it->second;
  };
  std::vector<int32_t> rows((size_t)nlist);
  for (int64_t i = 0; i < nlist; ++i) {
    const int64_t j = i + (int64_t)rng.below((uint32_t)(n - i));
    const int64_t vi = at(i), vj = at(j);
    rows[(size_t)i] = (int32_t)vj;
    moved[j] = vi;
  }
  return rows;
}

struct Scratch {
  int *assign, *perm, *hist;
  long long* sizes;
  float* norms;
};

Scratch take_scratch(Ctx& c, int64_t n, int64_t nlist, hipStream_t s) {
  Scratch w;
  w.assign = c.buf<int>("km.assign", (size_t)n, s);
  w.perm = c.buf<int>("km.perm", (size_t)n, s);
  w.hist = c.buf<int>("km.hist", (size_t)kmeans_sort_blocks(n) * nlist, s);
  w.sizes = c.buf<long long>("km.sizes", (size_t)nlist, s);
  w.norms = c.buf<float>("km.norms", (size_t)nlist, s);
  return w;
}

void check_kmeans_args(const float* x, int64_t n, int d, int64_t nlist, const char* what) {
  if (!x || n < 1 || n >= (int64_t(1) << 31)) throw Error(RVCX_E_INVALID, std::string(what) + ": bad x / n");
  if (nlist < 1 || nlist >= (int64_t(1) << 31)) throw Error(RVCX_E_INVALID, std::string(what) + ": nlist out of range");
  if (!kmeans_shape_ok(d))
    throw Error(RVCX_E_SHAPE, std::string(what) + ": d must be a multiple of 32 up to 1024 (got " +
                                  std::to_string(d) + ")");
  if (reinterpret_cast<uintptr_t>(x) & 15) throw Error(RVCX_E_INVALID, std::string(what) + ": x is not 16-byte aligned");
}

}  // namespace

void kmeans_assign_run(Ctx& c, const float* x, int64_t n, int d, const float* cent, int64_t nlist, int32_t* assign,
                       float* dist, hipStream_t s) {
  check_kmeans_args(x, n, d, nlist, "kmeans_assign");
  if (!cent || !assign || (reinterpret_cast<uintptr_t>(cent) & 15))
    throw Error(RVCX_E_INVALID, "kmeans_assign: bad centroid / output pointer");
  float* norms = c.buf<float>("km.norms", (size_t)nlist, s);
  check(kmeans_assign(x, n, d, cent, nlist, norms, assign, dist, s), "kmeans_assign");
}

void kmeans_update_run(Ctx& c, const float* x, int64_t n, int d, const int32_t* assign, int64_t nlist, float* cent,
                       int64_t* sizes, hipStream_t s) {
  check_kmeans_args(x, n, d, nlist, "kmeans_update");
  if (!cent || !assign) throw Error(RVCX_E_INVALID, "kmeans_update: bad centroid / assignment pointer");
  Scratch w = take_scratch(c, n, nlist, s);
  long long* off = c.buf<long long>("km.off", (size_t)nlist + 1, s);
  check(kmeans_sort(assign, n, nlist, w.hist, w.sizes, off, w.perm, s), "kmeans_sort");
  check(kmeans_update(x, d, w.perm, off, nlist, cent, s), "kmeans_update");
  if (sizes)
    RVCX_HIP(hipMemcpyAsync(sizes, w.sizes, (size_t)nlist * sizeof(long long), hipMemcpyDeviceToDevice, s));
}

void index_build(Ctx& c, const float* x, int64_t n, int d, int64_t nlist, const rvcx_index_build_opts& o,
                 hipStream_t s) {
  if (!x || n < 1 || n >= (int64_t(1) << 31)) throw Error(RVCX_E_INVALID, "index_build: bad x / n");
  if (nlist < 1 || nlist > n)
    throw Error(RVCX_E_INVALID, "index_build: nlist " + std::to_string(nlist) + " not in 1.." + std::to_string(n));
  if (o.niter < 0) throw Error(RVCX_E_INVALID, "index_build: niter must be >= 0");
  if (o.nprobe < 1) throw Error(RVCX_E_INVALID, "index_build: nprobe must be >= 1");
  // d: what the k-means kernels take and what index_load accepts back
  if (!kmeans_shape_ok(d) || d % 64 != 0)
    throw Error(RVCX_E_SHAPE, "index_build: d must be a multiple of 64 up to 1024 (got " + std::to_string(d) + ")");
  if (reinterpret_cast<uintptr_t>(x) & 15) throw Error(RVCX_E_INVALID, "index_build: x is not 16-byte aligned");

  // 1. initial centroids: nlist distinct rows
  std::vector<int32_t> rows;
  if (o.init_rows) {
    rows.resize((size_t)nlist);
    std::vector<int64_t> sorted(o.init_rows, o.init_rows + nlist);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= n) throw Error(RVCX_E_INVALID, "index_build: init_rows out of range");
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
      throw Error(RVCX_E_INVALID, "index_build: init_rows holds a row twice");
    for (int64_t i = 0; i < nlist; ++i) rows[(size_t)i] = (int32_t)o.init_rows[i];
  } else {
    rows = seeded_rows(n, nlist, o.seed);
  }

  // the index storage belongs to the context (as index_load's); the loaded index is replaced only at the end
  auto ix = std::make_unique<IvfIndex>();
  dev_alloc(ix->cent, (size_t)nlist * d * sizeof(float));
  dev_alloc(ix->vecs, (size_t)n * d * sizeof(float));
  dev_alloc(ix->off, (size_t)(nlist + 1) * sizeof(long long));
  dev_alloc(ix->ids, (size_t)n * sizeof(long long));
  dev_alloc(ix->slot_of_id, (size_t)n * sizeof(int));
  float* cent = static_cast<float*>(ix->cent.p);
  long long* off = static_cast<long long*>(ix->off.p);
  Scratch w = take_scratch(c, n, nlist, s);
  int32_t* d_rows = c.buf<int32_t>("km.rows", (size_t)nlist, s);
  RVCX_HIP(hipMemcpyAsync(d_rows, rows.data(), (size_t)nlist * sizeof(int32_t), hipMemcpyHostToDevice, s));
  check(gather_rows(x, d, d_rows, cent, (int)nlist, d, s), "index_build: initial centroids");
  RVCX_HIP(hipStreamSynchronize(s));  // `rows` is pageable host memory

  // 2. / 3. Lloyd iterations with faiss's split of empty lists (one synchronisation per iteration)
  std::vector<long long> hs((size_t)nlist);
  const float eps = 1.f / 1024.f;
  for (int it = 0; it < o.niter; ++it) {
    check(kmeans_assign(x, n, d, cent, nlist, w.norms, w.assign, nullptr, s), "kmeans_assign");
    check(kmeans_sort(w.assign, n, nlist, w.hist, w.sizes, off, w.perm, s), "kmeans_sort");
    check(kmeans_update(x, d, w.perm, off, nlist, cent, s), "kmeans_update");
    RVCX_HIP(hipMemcpyAsync(hs.data(), w.sizes, (size_t)nlist * sizeof(long long), hipMemcpyDeviceToHost, s));
    RVCX_HIP(hipStreamSynchronize(s));
    for (int64_t i = 0; i < nlist; ++i) {
      if (hs[(size_t)i] != 0) continue;
      const int64_t j = std::max_element(hs.begin(), hs.end()) - hs.begin();  // the first of the largest
      if (hs[(size_t)j] < 2) break;  // nothing left to split (faiss never splits a list of one)
      check(kmeans_split(cent, d, i, j, eps, s), "kmeans_split");
      hs[(size_t)i] = hs[(size_t)j] / 2;
      hs[(size_t)j] -= hs[(size_t)i];
    }
  }

  // 5. IndexIVF::add with ids 0..n-1: the final assignment, lists ascending by id
  check(kmeans_assign(x, n, d, cent, nlist, w.norms, w.assign, nullptr, s), "kmeans_assign");
  check(kmeans_sort(w.assign, n, nlist, w.hist, w.sizes, off, w.perm, s), "kmeans_sort");
  check(kmeans_pack(x, n, d, w.perm, static_cast<float*>(ix->vecs.p), static_cast<long long*>(ix->ids.p),
                    static_cast<int*>(ix->slot_of_id.p), s),
        "kmeans_pack");
  ix->off_host.resize((size_t)nlist + 1);
  RVCX_HIP(hipMemcpyAsync(ix->off_host.data(), off, (size_t)(nlist + 1) * sizeof(long long), hipMemcpyDeviceToHost, s));
  RVCX_HIP(hipStreamSynchronize(s));
  if (ix->off_host[(size_t)nlist] != n) throw Error(RVCX_E_HIP, "index_build: the lists do not hold every row");

  // 6. install, as index_load leaves it
  IvfView& v = ix->view;
  v.d = d;
  v.nlist = nlist;
  v.ntotal = n;
  v.nprobe = (int)std::min<int64_t>(o.nprobe, nlist);
  v.cent = cent;
  v.vecs = static_cast<const float*>(ix->vecs.p);
  v.off = off;
  v.ids = static_cast<const long long*>(ix->ids.p);
  v.slot_of_id = static_cast<const int*>(ix->slot_of_id.p);
  RVCX_HIP(hipDeviceSynchronize());  // no earlier call still reads the index this one replaces
  c.ivf = std::move(ix);
}

void index_centroids(Ctx& c, float* out, hipStream_t s) {
  if (!c.ivf) throw Error(RVCX_E_STATE, "no feature index loaded");
  const IvfView& v = c.ivf->view;
  RVCX_HIP(hipMemcpyAsync(out, v.cent, (size_t)v.nlist * v.d * sizeof(float), hipMemcpyDeviceToDevice, s));
}

// faiss 1.7.4 write_index(IndexIVFFlat): the layout parse_ivf reads (index_ivf.cpp), with direct map type 0
int64_t index_save(Ctx& c, void* bytes, int64_t cap) {
  if (!c.ivf) throw Error(RVCX_E_STATE, "no feature index loaded");
  const IvfIndex& ix = *c.ivf;
  const IvfView& v = ix.view;
  const std::vector<long long>& off = ix.off_host;
  const uint64_t nlist = (uint64_t)v.nlist, d = (uint64_t)v.d, ntotal = (uint64_t)v.ntotal;
  uint64_t non_empty = 0;
  for (uint64_t l = 0; l < nlist; ++l) non_empty += off[l + 1] > off[l] ? 1 : 0;
  // ArrayInvertedLists: "full" sizes, or "sprs" (list, size) pairs; a loaded file keeps its own (IvfIndex::size_enc)
  const bool full = ix.size_enc < 0 ? non_empty > nlist / 2 : ix.size_enc == 0;
  const uint64_t hdr = 4 + 8 + 8 + 8 + 1 + 4;
  const uint64_t total = 4 + hdr + 16 + 4 + hdr + 8 + nlist * d * 4 + 1 + 8 + 4 + 16 + 4 + 8 +
                         (full ? nlist * 8 : non_empty * 16) + ntotal * (d * 4 + 8);
  if (!bytes) return (int64_t)total;
  if (cap < 0 || (uint64_t)cap < total)
    throw Error(RVCX_E_CAPACITY, "index_save: " + std::to_string(total) + " B needed, " + std::to_string(cap) + " given");
  uint8_t* p = static_cast<uint8_t*>(bytes);
  auto put = [&](const void* src, size_t k) {
    std::memcpy(p, src, k);
    p += k;
  };
  auto put_u64 = [&](uint64_t x) { put(&x, 8); };
  auto put_header = [&](int32_t dd, int64_t nt) {  // write_index_header
    const int64_t dummy = int64_t(1) << 20;
    const uint8_t trained = 1;
    const int32_t metric = 1;  // METRIC_L2
    put(&dd, 4);
    put(&nt, 8);
    put(&dummy, 8);
    put(&dummy, 8);
    put(&trained, 1);
    put(&metric, 4);
  };
  RVCX_HIP(hipSetDevice(c.device));
  RVCX_HIP(hipDeviceSynchronize());
  put("IwFl", 4);
  put_header((int32_t)d, (int64_t)ntotal);
  put_u64(nlist);
  put_u64((uint64_t)v.nprobe);
  put("IxF2", 4);
  put_header((int32_t)d, (int64_t)nlist);
  put_u64(nlist * d);
  RVCX_HIP(hipMemcpy(p, v.cent, nlist * d * 4, hipMemcpyDeviceToHost));
  p += nlist * d * 4;
  const uint8_t dm_type = 0;  // DirectMap::NoMap
  put(&dm_type, 1);
  put_u64(0);
  put("ilar", 4);
  put_u64(nlist);
  put_u64(d * 4);
  if (full) {
    put("full", 4);
    put_u64(nlist);
    for (uint64_t l = 0; l < nlist; ++l) put_u64((uint64_t)(off[l + 1] - off[l]));
  } else {
    put("sprs", 4);
    put_u64(non_empty * 2);
    for (uint64_t l = 0; l < nlist; ++l)
      if (off[l + 1] > off[l]) {
        put_u64(l);
        put_u64((uint64_t)(off[l + 1] - off[l]));
      }
  }
  for (uint64_t l = 0; l < nlist; ++l) {  // per non-empty list: codes, then ids
    const uint64_t a = (uint64_t)off[l], cnt = (uint64_t)(off[l + 1] - off[l]);
    if (!cnt) continue;
    RVCX_HIP(hipMemcpy(p, v.vecs + a * d, cnt * d * 4, hipMemcpyDeviceToHost));
    p += cnt * d * 4;
    RVCX_HIP(hipMemcpy(p, v.ids + a, cnt * 8, hipMemcpyDeviceToHost));
    p += cnt * 8;
  }
  if ((uint64_t)(p - static_cast<uint8_t*>(bytes)) != total) throw Error(RVCX_E_HIP, "index_save: size mismatch");
  return (int64_t)total;
}

}  // namespace rvcx
