// The runtime's side of a conv launch: plan (conv_dispatch.hip), weight image, split-K slab, run, with optional event
// timing; the fused ResBlock pair's launch; and the context's streams, events, device-status word and packed weights.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "runtime.h"

namespace rvcx {
hipStream_t Ctx::aux_stream() {
  if (!aux) {
    RVCX_HIP(hipSetDevice(device));
    // (the aux stream at the device's least priority measured neutral: 18.22 vs 18.19 ms, round 3)
    RVCX_HIP(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
    RVCX_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    RVCX_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    RVCX_HIP(hipEventCreateWithFlags(&ev_gate, hipEventDisableTiming));
  }
  return aux;
}

unsigned* Ctx::device_status() {
  if (!status_host) {
    RVCX_HIP(hipSetDevice(device));
    void* h = nullptr;
    RVCX_HIP(hipHostMalloc(&h, 64, hipHostMallocMapped));
    std::memset(h, 0, 64);
    status_host = static_cast<unsigned*>(h);
    void* d = nullptr;
    RVCX_HIP(hipHostGetDevicePointer(&d, h, 0));
    status_dev = static_cast<unsigned*>(d);
  }
  return status_dev;
}

void Ctx::check_device_status() {
  if (!status_host) return;
  const unsigned v = __atomic_load_n(status_host, __ATOMIC_ACQUIRE);
  if (v == 0) return;
  __atomic_store_n(status_host, 0u, __ATOMIC_RELEASE);
  std::string what;
  if (v & 1u) what += "gru: partner hand-off timed out (the RMVPE BiGRU's workgroups were not co-resident); ";
  throw Error(RVCX_E_HIP, what + "the outputs of the call that raised this flag are invalid");
}

Ctx::~Ctx() {
  if (status_host) (void)hipHostFree(status_host);
  for (auto& kv : call_ev)
    if (kv.second) (void)hipEventDestroy(kv.second);
  if (aux) {
    (void)hipStreamSynchronize(aux);
    (void)hipEventDestroy(ev_fork);
    (void)hipEventDestroy(ev_join);
    (void)hipEventDestroy(ev_gate);
    (void)hipStreamDestroy(aux);
  }
}

hipStream_t fork_aux(Ctx& c, hipStream_t s) {
  static const bool no_overlap = [] {
    const char* e = rvcx_knob("RVCX_NO_OVERLAP");
    return e && std::atoi(e) != 0;
  }();
  if (c.prof || no_overlap) return s;
  hipStream_t ax = c.aux_stream();
  RVCX_HIP(hipEventRecord(c.ev_fork, s));
  RVCX_HIP(hipStreamWaitEvent(ax, c.ev_fork, 0));
  return ax;
}

void join_aux(Ctx& c, hipStream_t s, hipStream_t ax) {
  if (ax == s) return;
  RVCX_HIP(hipEventRecord(c.ev_join, ax));
  RVCX_HIP(hipStreamWaitEvent(s, c.ev_join, 0));
}

float* Ctx::W(const std::string& name) const {
  auto it = sdev.find(name);
  if (it == sdev.end()) {
    it = dev.find(name);
    if (it == dev.end()) throw Error(RVCX_E_STATE, "packed weight not found: " + name);
  }
  return static_cast<float*>(it->second->p);
}

int Ctx::new_voice() {
  const int id = next_voice++;
  voices.emplace(id, Voice());
  return id;
}

// The members that make up the current voice change places with a parked entry. Twice per select: the current state
// into its own (hollow) entry, then the chosen entry's state into the members.
static void swap_voice(Ctx& c, Voice& v) {
  std::swap(c.scfg, v.scfg);
  std::swap(c.synth_cfg_set, v.synth_cfg_set);
  c.host[RVCX_MODEL_SYNTH].swap(v.host);
  c.sdev.swap(v.sdev);
  c.ups.swap(v.ups);
  c.ivf.swap(v.ivf);
  std::swap(c.ready[RVCX_MODEL_SYNTH], v.ready);
}

void Ctx::select_voice(int id) {
  if (id == cur_voice) return;
  auto it = voices.find(id);
  if (it == voices.end()) throw Error(RVCX_E_INVALID, "voice " + std::to_string(id) + " does not exist (or was freed)");
  swap_voice(*this, voices.at(cur_voice));
  swap_voice(*this, it->second);
  cur_voice = id;
}

void Ctx::voice_bytes(int id, int64_t* weight_bytes, int64_t* split_bytes) {
  if (!has_voice(id)) throw Error(RVCX_E_INVALID, "voice " + std::to_string(id) + " does not exist (or was freed)");
  const auto& m = id == cur_voice ? sdev : voices.at(id).sdev;
  int64_t wb = 0, sb = 0;
  for (const auto& kv : m) {
    wb += (int64_t)kv.second->bytes;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(kv.second->p), hi = lo + kv.second->bytes;
    for (const auto& e : wsplit_cache) {
      const uintptr_t u = reinterpret_cast<uintptr_t>(std::get<0>(e.first));
      if (u >= lo && u < hi && e.second) sb += (int64_t)e.second->bytes;
    }
    for (const auto& e : rb_wsplit_cache) {
      const uintptr_t u = reinterpret_cast<uintptr_t>(e.first.first);
      if (u >= lo && u < hi && e.second) sb += (int64_t)e.second->bytes;
    }
  }
  if (weight_bytes) *weight_bytes = wb;
  if (split_bytes) *split_bytes = sb;
}

void Ctx::free_voice(int id) {
  if (!has_voice(id)) throw Error(RVCX_E_INVALID, "voice " + std::to_string(id) + " does not exist (or was freed)");
  if (id == 0 || id == cur_voice) throw Error(RVCX_E_STATE, "voice 0 and the current voice cannot be freed");
  RVCX_HIP(hipDeviceSynchronize());
  Voice& v = voices.at(id);
  for (const auto& kv : v.sdev) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(kv.second->p);
    wranges.erase(lo);
    drop_splits(lo, lo + kv.second->bytes);
  }
  voices.erase(id);  // the tensors and the index go with the entry
}

float* Ctx::alloc_weight(const std::string& name, const std::vector<float>& data) {
  std::unique_ptr<DevBuf> b(new DevBuf());
  size_t bytes = data.size() * sizeof(float);
  if (bytes == 0) bytes = 16;
  if (hipMalloc(&b->p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    throw Error(RVCX_E_OOM, "weight allocation failed: " + name);
  }
  b->bytes = bytes;
  RVCX_HIP(hipMemcpy(b->p, data.data(), data.size() * sizeof(float), hipMemcpyHostToDevice));
  float* p = static_cast<float*>(b->p);
  auto& dev = packing_synth ? sdev : this->dev;  // the current voice's tensors, or the shared models'
  auto old = dev.find(name);
  if (old != dev.end()) {
    const uintptr_t o = reinterpret_cast<uintptr_t>(old->second->p);
    wranges.erase(o);
    drop_splits(o, o + old->second->bytes);  // the replaced tensor's split images
  }
  const uintptr_t u = reinterpret_cast<uintptr_t>(p);
  drop_splits(u, u + bytes);  // images cached for an earlier tensor at a reused address
  wranges[u] = u + bytes;
  dev[name] = std::move(b);
  return p;
}

void Ctx::drop_splits(uintptr_t lo, uintptr_t hi) {
  for (auto it = wsplit_cache.begin(); it != wsplit_cache.end();) {
    const uintptr_t u = reinterpret_cast<uintptr_t>(std::get<0>(it->first));
    it = (u >= lo && u < hi) ? wsplit_cache.erase(it) : std::next(it);
  }
  for (auto it = rb_wsplit_cache.begin(); it != rb_wsplit_cache.end();) {
    const uintptr_t u = reinterpret_cast<uintptr_t>(it->first.first);
    it = (u >= lo && u < hi) ? rb_wsplit_cache.erase(it) : std::next(it);
  }
}

bool Ctx::is_weight(const void* q) const {
  const uintptr_t u = reinterpret_cast<uintptr_t>(q);
  auto it = wranges.upper_bound(u);
  if (it == wranges.begin()) return false;
  --it;
  return u < it->second;
}

// the weight tensor's pre-split image (built once on first use; the stream then synchronises so a later use on
// another stream never races the build)
const void* Ctx::wsplit_for(const ConvArgs& a, hipStream_t s) {
  const auto key = std::make_tuple(static_cast<const void*>(a.w), a.ldw, a.w_ts, a.N, a.C_in, a.taps, a.wsplit_fmt);
  auto& slot = wsplit_cache[key];
  if (!slot) {
    std::unique_ptr<DevBuf> b(new DevBuf());
    const size_t bytes = (size_t)conv_wsplit_bytes(a);
    if (hipMalloc(&b->p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      throw Error(RVCX_E_OOM, "split-weight allocation failed");
    }
    b->bytes = bytes;
    check(conv_wsplit_build(a, b->p, s), "conv_wsplit_build");
    RVCX_HIP(hipStreamSynchronize(s));
    slot = std::move(b);
  }
  return slot->p;
}

const void* Ctx::rb_wsplit_for(const float* w, int C, int k, int wfmt, hipStream_t s) {
  auto& slot = rb_wsplit_cache[{static_cast<const void*>(w), wfmt}];
  if (!slot) {
    std::unique_ptr<DevBuf> b(new DevBuf());
    const size_t bytes = (size_t)rb_wsplit_bytes(C, k, wfmt);
    if (hipMalloc(&b->p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      throw Error(RVCX_E_OOM, "split-weight allocation failed");
    }
    b->bytes = bytes;
    check(rb_wsplit_build(w, C, k, b->p, s, wfmt), "rb_wsplit_build");
    RVCX_HIP(hipStreamSynchronize(s));
    slot = std::move(b);
  }
  return slot->p;
}

// a timing event from the context's pool (rvcx_profile_read* hands them back)
static hipEvent_t take_event(Ctx& c) {
  hipEvent_t e;
  if (!c.prof_pool.empty()) {
    e = c.prof_pool.back();
    c.prof_pool.pop_back();
  } else {
    RVCX_HIP(hipEventCreate(&e));
  }
  return e;
}

void launch_rb_pair(Ctx& c, const RbPairArgs& a, hipStream_t s) {
  constexpr int cfg = 0;
  if (!c.prof) {
    check(rb_pair(a, cfg, s), "rb_pair");
    return;
  }
  // algorithmic work: the two convs over the valid rows
  const double flops = 2.0 * 2.0 * a.B * (double)a.T * a.C * a.C * a.k;
  // x read, y written (+ read when accumulating), both weight tensors
  const double bytes = 4.0 * ((double)a.B * a.T * a.C * (2 + (a.acc_mode != ACC_STORE ? 1 : 0)) + 2.0 * a.k * a.C * a.C);
  Ctx::ProfRec r{take_event(c), take_event(c), flops, 0, a.T, a.C, a.C, -a.k, a.B, 1, bytes,
                 a.wfmt == RB_WF16 ? (a.lowp ? Ctx::PEAK_F16 : Ctx::PEAK_F16X2) : Ctx::PEAK_SPLIT};
  r.kind = CK_RBPAIR;
  RVCX_HIP(hipEventRecord(r.a, s));
  check(rb_pair(a, cfg, s), "rb_pair");
  RVCX_HIP(hipEventRecord(r.b, s));
  c.prof_recs.push_back(r);
}

bool conv_routes_wsb16(Ctx& c, const ConvArgs& a_in) {
  ConvArgs a = a_in;
  if (c.conv_math > 0 && a.math == 0) a.math = c.conv_math;
  const ConvPlan p = conv_plan(a, false, a.w_static || c.is_weight(a.w));
  return (p.kind == CK_WSB16 || p.kind == CK_WST) && p.wsplit_fmt == WSPLIT_H16 && p.ksplit == 1;
}

namespace {
// the planned launch: the slab, conv_run and, with kernel timing on, its record
void run_planned(Ctx& c, const ConvPlan& p, ConvArgs& a, bool two_d, bool forced, hipStream_t s, double flops) {
  // split-K slabs are per stream: the aux stream's convs run concurrently with the caller's
  if (p.ksplit > 1)
    a.ws = c.buf<float>(c.aux && s == c.aux ? "conv.splitk.aux" : "conv.splitk", (size_t)p.slab_floats, s);
  auto run = [&] {
    const hipError_t e = conv_run(p, a, two_d, s, forced);
    if (e == hipSuccess) return;
    // planned launches are not retried on another family: a refusal is a bug in the plan or a bad record
    auto n = [](long long v) { return std::to_string(v); };
    throw Error(RVCX_E_HIP, std::string(two_d ? "conv2d: " : "conv1d: ") + conv_kind_name(p.kind) + " tile " + n(p.tile) +
                                " ksplit " + n(p.ksplit) + " refused " + n(a.T_out) + " x " + n(a.W_out) + " rows, N " +
                                n(a.N) + ", C_in " + n(a.C_in) + ", " + n(a.taps) + " taps: " + hipGetErrorString(e));
  };
  if (!c.prof) return run();
  if (flops < 0) {
    const double M = two_d ? (double)a.T_out * a.W_out : (double)a.T_out;
    flops = 2.0 * M * a.N * (double)a.C_in * a.taps * a.batch * a.batch_inner;
  }
  // input rows read once, weights once, output written once (+ read again for a residual / accumulate)
  const double in_rows = two_d ? (double)a.T_in * a.W_in : (double)a.T_in;
  const double out_el = (two_d ? (double)a.T_out * a.W_out : (double)a.T_out) * a.N * a.batch * a.batch_inner;
  const double alg_bytes = 4.0 * (in_rows * a.C_in * a.batch * a.batch_inner + (double)a.taps * a.N * a.C_in +
                                  out_el * (1 + (a.res && a.res_mode != RES_NONE ? 1 : 0) +
                                            (a.acc_mode != ACC_STORE ? 1 : 0)));
  // the launch's arithmetic ceiling (the rest of the family is priced at the bf16 split's, a lower bound for the few
  // launches on the fp32-input MFMA)
  const bool wsb = p.kind == CK_WSB16 || p.kind == CK_WST;
  const double peak = p.wsplit_fmt == WSPLIT_H16 ? ((a.lowp && wsb) ? Ctx::PEAK_F16 : Ctx::PEAK_F16X2)
                      : (p.wsplit_fmt == WSPLIT_S2D && a.wsplit) ? Ctx::PEAK_F16X2
                                                                 : Ctx::PEAK_SPLIT;
  Ctx::ProfRec r{take_event(c), take_event(c), flops, two_d ? 1 : 0, two_d ? a.T_out * a.W_out : a.T_out, a.N, a.C_in,
                 a.taps, a.batch * a.batch_inner, p.ksplit, alg_bytes, peak};
  r.kind = p.kind;
  RVCX_HIP(hipEventRecord(r.a, s));
  run();
  RVCX_HIP(hipEventRecord(r.b, s));
  c.prof_recs.push_back(r);
}
}  // namespace

// plan, image, slab, run
void launch_conv(Ctx& c, const ConvArgs& a_in, bool two_d, hipStream_t s, double flops) {
  ConvArgs a = a_in;
  if (c.conv_math > 0 && a.math == 0) a.math = c.conv_math;
  const ConvPlan p = conv_plan(a, two_d, a.w_static || c.is_weight(a.w));
  if (p.needs_image) {
    a.wsplit_fmt = p.wsplit_fmt;  // the cache key and the builder read it
    a.wsplit = c.wsplit_for(a, s);
  }
  run_planned(c, p, a, two_d, false, s, flops);
}

ConvPlan launch_conv_test(Ctx& c, const ConvArgs& a_in, bool two_d, bool static_weight, const ConvForce& force,
                          int expect_kind, const char* who, hipStream_t s) {
  ConvArgs a = a_in;
  if (c.conv_math > 0 && a.math == 0) a.math = c.conv_math;
  const ConvPlan p = conv_plan(a, two_d, static_weight, force);
  const std::string w(who);
  const int want = force.kind >= 0 ? force.kind : expect_kind;
  if (p.kind == CK_OTHER || (expect_kind >= 0 && p.kind != expect_kind))
    throw Error(RVCX_E_SHAPE, w + ": " + (want >= 0 ? conv_kind_name(want) : "the size policy's family") + " does not "
                                  "admit this form, or its gate / LayerNorm get no split (two steps, no_splitk off)");
  // (the runtime fuses the noise conv only where conv_routes_wsb16 holds)
  if (a.nz_har && !((p.kind == CK_WSB16 || p.kind == CK_WST) && p.ksplit == 1))
    throw Error(RVCX_E_SHAPE, w + ": the fused noise conv needs an unsplit weight-streamed / weight-stationary launch");
  if (p.wsplit_fmt >= 0) {
    // a fresh image every call, never the address-keyed cache: the caller may reuse the weight's address (or torch's
    // allocator may hand it back) with new weights of the same shape
    a.wsplit_fmt = p.wsplit_fmt;
    void* img = c.buf<char>("conv.test.wsplit", (size_t)conv_wsplit_bytes(a), s);
    check(conv_wsplit_build(a, img, s), "conv_wsplit_build");
    a.wsplit = img;
  }
  run_planned(c, p, a, two_d, force.kind >= 0, s, -1.0);
  return p;
}

__global__ void k_set_i32(int32_t* p, int32_t v) { p[0] = v; }
void set_i32(int32_t* p, int32_t v, hipStream_t s) {
  hipLaunchKernelGGL(k_set_i32, dim3(1), dim3(1), 0, s, p, v);
  check(hipGetLastError(), "set_i32");
}
void set_i32_once(Ctx& c, const std::string& name, int32_t* p, int32_t v, hipStream_t s) {
  auto it = c.i32_marks.find(name);
  if (it != c.i32_marks.end() && it->second.first == p && it->second.second == v) return;
  set_i32(p, v, s);
  c.i32_marks[name] = {p, v};
}
}  // namespace rvcx

