// rvcx runtime internals: context, weight store, workspace.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/rvcx.h"
#include "rvcx_kernels.h"

namespace rvcx {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define RVCX_HIP(expr)                                                                                 \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess)                                                                              \
      throw ::rvcx::Error(RVCX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " at " +     \
                                          __FILE__ + ":" + std::to_string(__LINE__));                  \
  } while (0)

struct HostTensor {
  std::vector<float> v;
  std::vector<int64_t> shape;
  size_t numel() const { return v.size(); }
};

// Device buffer (owned).
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool borrowed = false;  // carved from the caller's workspace arena (rvcx_set_workspace): not freed here
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  // back to the empty state (frees an owned allocation)
  void reset() {
    if (p && !borrowed) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    borrowed = false;
  }
};

struct SynthCfg {
  int I = 192, H = 192, F = 768, n_heads = 2, n_layers = 6, ksize = 3;
  std::vector<int> rb_k{3, 7, 11};
  std::vector<std::vector<int>> rb_d{{1, 3, 5}, {1, 3, 5}, {1, 3, 5}};
  std::vector<int> ups{12, 10, 2, 2};
  int C0 = 512;
  std::vector<int> up_k{24, 20, 4, 4};
  int n_spk = 109, gin = 256, sr = 48000, emb_dim = 768;
  int window = 10, flow_k = 5, flow_layers = 3, flow_n = 4;
  bool f0 = true;   // pitch-guided (NSF decoders) or not (HiFiGANGenerator): synthesizers.py:84-139
  int vocoder = 0;  // 0 HiFi-GAN (NSF), 1 MRF HiFi-GAN, 2 RefineGAN (synthesizers.py:86-118)
  int upp() const {
    int u = 1;
    for (int x : ups) u *= x;
    return u;
  }
  // harmonics of the decoder's source: NSF 1 (harmonic_num 0), MRF 9 (synthesizers.py:95), RefineGAN 1
  int src_harmonics() const { return vocoder == 1 ? 9 : 1; }
  // floats of injected source noise per batch row of T frames (the decoder's randn_like / rand draws):
  // NSF [T*upp]; MRF / RefineGAN [T*upp][H] noise, the B x H initial phases of all rows follow the B rows
  long long src_noise_row(long long T) const { return f0 ? T * upp() * src_harmonics() : 0; }
  long long src_noise_tail() const { return (f0 && vocoder != 0) ? src_harmonics() : 0; }
  // every injected decoder draw of a B x T call (RefineGAN adds its AdaIN noise: runtime_refinegan.cpp)
  long long src_noise_total(int B, long long T) const;
};

// FCPE hyper-parameters: config["mel"] / config["model"] of an FCPE checkpoint (FCPE.py:731-756, rvcx_fcpe_desc)
struct FcpeCfg {
  int sr = 16000, n_fft = 1024, win = 1024, hop = 160, n_mels = 128;
  double fmin = 0.0, fmax = 8000.0;
  int n_layers = 6, n_chans = 512, out_dims = 360;
  int n_heads = 8, dim_head = 64;  // SelfAttention's defaults (FCPE.py:466-468), fixed in FCPE
  int n_feat = 0;                  // projection_matrix rows, from the weights (finalize_fcpe)
  int conv_k = 31;                 // ConformerConvModule's depthwise kernel (FCPE.py:329)
};

// ConvTranspose1d lowered to a polyphase conv: input row for output q, tap t is q + t - pad.
struct UpsLayer {
  int cin = 0, cout = 0, u = 0, k = 0, taps = 0, pad = 0;
  float* w = nullptr;     // [taps][u*cout][cin]
  float* b = nullptr;     // [u*cout]
};

// FAISS IndexIVFFlat resident in HBM (index_ivf.cpp; layout in ivf.hip)
struct IvfIndex {
  IvfView view;
  DevBuf cent, vecs, off, ids, slot_of_id;
  std::vector<long long> off_host;  // off [nlist + 1] on the host too: the list sizes index_save writes
  // how index_save encodes the list sizes: -1 faiss's own choice ("full" when more than nlist / 2 lists are
  // non-empty, else "sprs": a built index), 0 / 1 "full" / "sprs" as the loaded file had them, so that a loaded
  // file saves back byte for byte whichever its writer chose
  int size_enc = -1;
};

// A voice: everything that differs between two RVC checkpoints. The context's members of the same names hold the
// current voice; the other voices of the bank are parked in Ctx::voices and change places with them on select_voice
// (map and vector swaps on the host: no device call, no copy of weight data).
struct Voice {
  SynthCfg scfg;
  bool synth_cfg_set = false;
  std::map<std::string, HostTensor> host;                // the uploaded synthesizer tensors (Ctx::host[0])
  std::map<std::string, std::unique_ptr<DevBuf>> sdev;  // their packed images
  std::vector<UpsLayer> ups;
  std::unique_ptr<IvfIndex> ivf;
  bool ready = false;
};

// what two voices must share to be served by one stream group or one batch: the quantities that fix the buffer
// geometry, the HuBERT version and the layouts of injected noise
struct VoiceGeom {
  int sr = 0, upp = 0, emb_dim = 0, I = 0, f0 = 0, vocoder = 0;
  bool operator==(const VoiceGeom& o) const {
    return sr == o.sr && upp == o.upp && emb_dim == o.emb_dim && I == o.I && f0 == o.f0 && vocoder == o.vocoder;
  }
};
inline VoiceGeom voice_geom(const SynthCfg& g) { return {g.sr, g.upp(), g.emb_dim, g.I, g.f0 ? 1 : 0, g.vocoder}; }

struct Ctx {
  int device = 0;
  std::string err;
  SynthCfg scfg;
  bool synth_cfg_set = false;
  FcpeCfg fcfg;
  std::map<std::string, HostTensor> host[5];  // synth, hubert, rmvpe, crepe, fcpe
  std::map<std::string, std::unique_ptr<DevBuf>> dev;  // packed weights of the shared models
  // packed weights of the current voice's synthesizer (finalize_synth packs into it: packing_synth); W looks here first
  std::map<std::string, std::unique_ptr<DevBuf>> sdev;
  bool packing_synth = false;
  bool ready[5] = {false, false, false, false, false};
  std::vector<UpsLayer> ups;
  // the voice bank: voice 0 exists from the start and is current. voices holds every live id; the current voice's entry
  // is hollow (its state is in the members above). Ids are never reused.
  std::map<int, Voice> voices;
  int cur_voice = 0, next_voice = 1;
  Ctx() { voices[0]; }
  bool has_voice(int id) const { return voices.count(id) != 0; }
  int new_voice();
  void select_voice(int id);  // host only; throws RVCX_E_INVALID for an unknown or freed id
  void free_voice(int id);    // synchronises the device; RVCX_E_STATE for voice 0 and the current voice
  // bytes of a voice's packed tensors, and of the pre-split images built from them so far
  void voice_bytes(int id, int64_t* weight_bytes, int64_t* split_bytes);
  // pipeline high-pass (rvc/infer/pipeline.py:22-27), normalised so a[0] = 1
  int hp_order = 0;
  std::vector<double> hp_b, hp_a, hp_zi;
  // the same filter as second-order sections (rvcx_set_highpass_sos): chunk-parallel scan (iir_scan.hip)
  SosPlan hp_sos;
  DevBuf hp_sos_buf;
  // workspace pool
  std::map<std::string, std::unique_ptr<DevBuf>> ws;
  uint64_t call_counter = 0;
  // kernel timing (rvcx_profile): event pairs around every conv-GEMM launch, on its stream
  bool prof = false;
  int conv_math = 0;  // ConvArgs::math of every conv launch (rvcx_set_conv_math): 0 default, 1 fp32 MFMA, 2 split
  // the arithmetic a launch without ConvArgs::math gets: rvcx_set_conv_math, else RVCX_CONV_MATH
  int conv_math_default() const {
    return rvcx::conv_math(conv_math);
  }
  static constexpr double PEAK_SPLIT = 2500.0 / 6.0, PEAK_F16X2 = 2500.0 / 3.0, PEAK_F16 = 2500.0;
  struct ProfRec {
    hipEvent_t a, b;
    double flops;
    int two_d, M, N, C_in, taps, batch, ksplit;  // shape, for RVCX_PROF_DUMP
    double bytes;  // algorithmic HBM bytes: operands read once, result written once (RVCX_PROF_DUMP)
    double peak_tf;  // the MFMA ceiling of the launch's arithmetic, algorithmic fp32 TFLOP/s
    int kind = CK_OTHER;  // the kernel family that ran (ConvKind)
  };
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> prof_pool;
  std::unique_ptr<IvfIndex> ivf;  // speaker-embedding index (optional)
  // pre-split weight images of the weight-streamed conv kernel, per (weight, layout); an entry is dropped when its
  // weight tensor is re-packed (alloc_weight), so finalizing one model keeps the other models' images
  std::map<std::tuple<const void*, int, long long, int, int, int, int>, std::unique_ptr<DevBuf>> wsplit_cache;
  const void* wsplit_for(const ConvArgs& a, hipStream_t s);
  // pre-split images of the fused ResBlock pair kernel (resblock_fused.hip), per weight tensor
  std::map<std::pair<const void*, int>, std::unique_ptr<DevBuf>> rb_wsplit_cache;
  const void* rb_wsplit_for(const float* w, int C, int k, int wfmt, hipStream_t s);
  // the pipelines and the streaming hop hand the synthesizer the output window their trim keeps (DecWindow below);
  // off: the generator runs full-length (rvcx_set_dec_window; RVCX_DEC_WINDOW=0 at context creation). Same outputs.
  // The arena query (pipeline_workspace_bytes) passes no window either: it plans the worst case.
  bool dec_window = true;
  // second stream for work independent of the caller's stream (HuBERT beside RMVPE), created lazily
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_gate = nullptr;
  hipStream_t aux_stream();
  // device-side fault flags in pinned host-mapped memory (bit 0: a BiGRU partner hand-off timed out).
  // Kernels store into it; the host reads it after a synchronisation: every compute entry point checks
  // it on entry (faults of earlier, completed calls), the pipeline at its own sync points, and
  // rvcx_device_status after synchronising the caller's stream.
  // buffers whose zero parts survive from call to call (the BiGRU hand-off tags, the NSF source's pad columns): zeroed
  // only when the buffer or its layout changes, not by a fill launch every call
  std::map<std::string, std::pair<const void*, long long>> zero_marks;
  // small device scalars written from the host (the synthesizer's length / speaker id): the launch is skipped when the
  // named buffer already holds the value (C2 writes the same two every call)
  std::map<std::string, std::pair<const void*, int32_t>> i32_marks;
  // returns true when it zeroed
  bool zero_once(const std::string& name, void* p, size_t bytes, long long layout, hipStream_t s) {
    auto& m = zero_marks[name];
    if (m.first == p && m.second == layout) return false;
    RVCX_HIP(hipMemsetAsync(p, 0, bytes, s));
    m = {p, layout};
    return true;
  }
  // the BiGRU hand-off tag counter of each zeroed xchg slice (gru_bidir), reset whenever the buffer is re-zeroed
  std::map<const void*, unsigned> gru_tags;
  unsigned* status_host = nullptr;
  unsigned* status_dev = nullptr;
  unsigned* device_status();
  void check_device_status();  // throws Error(RVCX_E_HIP, ...) and clears the flags when any is set
  ~Ctx();

  float* W(const std::string& name) const;
  // address ranges of the packed weights (alloc_weight): a contraction whose B operand lies in one is static
  std::map<uintptr_t, uintptr_t> wranges;
  bool is_weight(const void* p) const;
  // forget the split images cached for weights in [lo, hi) (a tensor replaced or an address reused)
  void drop_splits(uintptr_t lo, uintptr_t hi);
  float* alloc_weight(const std::string& name, const std::vector<float>& data);
  template <class T>
  T* buf(const std::string& name, size_t count, hipStream_t s);
  // caller-owned workspace arena (rvcx_set_workspace): the named pool is carved from it (256-B aligned, bump order)
  // instead of hipMalloc; a buffer that has to grow takes a new region; past the end a call fails with RVCX_E_OOM
  char* arena = nullptr;
  size_t arena_bytes = 0, arena_used = 0;
  size_t carved = 0;  // bytes the pool has taken since the last release (every region, regrown ones included)
  // Call-to-call ordering: every compute entry point starts with begin_call(), which records an event on
  // each stream the previous call took pool buffers on; the first pool buffer a call takes on a stream makes that
  // stream wait for the previous call's events on OTHER streams. A call on stream B therefore never overwrites a
  // region (arena mode: the same offsets under other names; pool mode: the same named buffers) that a call still
  // running on stream A uses; calls on one stream stay ordered by the stream itself (no wait is issued).
  std::vector<hipStream_t> call_streams;                              // streams the current call took buffers on
  std::vector<std::pair<hipStream_t, hipEvent_t>> prev_call_events;  // the previous call's, recorded at begin_call
  std::map<hipStream_t, hipEvent_t> call_ev;                           // one reusable event per stream
  void begin_call() {
    prev_call_events.clear();
    for (hipStream_t st : call_streams) {
      hipEvent_t& e = call_ev[st];
      if (!e) RVCX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      RVCX_HIP(hipEventRecord(e, st));
      prev_call_events.emplace_back(st, e);
    }
    call_streams.clear();
    arena_rewind();
  }
  void touch_stream(hipStream_t s) {
    for (hipStream_t st : call_streams)
      if (st == s) return;
    call_streams.push_back(s);
    for (const auto& pe : prev_call_events)
      if (pe.first != s) RVCX_HIP(hipStreamWaitEvent(s, pe.second, 0));
  }
  // Arena mode: every API call carves its regions from offset 0 again (begin_call, before any work), so a call never
  // inherits the regions earlier calls regrew; reuse is ordered by the caller's stream and, across streams, by
  // begin_call's events. The marks describing buffer contents go with the regions (a caller that wrote into its arena
  // between calls cannot leave a stale zeroed buffer or memoised scalar behind).
  void arena_rewind() {
    if (arena) drop_pool();
  }
  // drop the named pool, with the marks that describe its contents (zeroed buffers, memoised scalars, BiGRU tag
  // counters)
  void drop_pool() {
    ws.clear();
    zero_marks.clear();
    i32_marks.clear();
    gru_tags.clear();
    arena_used = 0;
    carved = 0;
  }
  // synchronise the device, then drop the pool
  void release_pool() {
    RVCX_HIP(hipDeviceSynchronize());
    drop_pool();
  }
  size_t pool_bytes() const {
    size_t t = 0;
    for (const auto& kv : ws) t += kv.second ? kv.second->bytes : 0;
    return t;
  }
};

// A call that serves several voices selects each in turn (host only) and leaves the context's current voice as it
// found it, on an exception too. A voice freed meanwhile cannot be the one to return to: the current voice is never freed.
struct VoiceScope {
  Ctx& c;
  int saved;
  explicit VoiceScope(Ctx& ctx) : c(ctx), saved(ctx.cur_voice) {}
  ~VoiceScope() { c.select_voice(saved); }
  VoiceScope(const VoiceScope&) = delete;
  VoiceScope& operator=(const VoiceScope&) = delete;
};

template <class T>
T* Ctx::buf(const std::string& name, size_t count, hipStream_t s) {
  size_t bytes = count * sizeof(T);
  if (bytes == 0) bytes = 16;
  bytes = (bytes + 255) & ~size_t(255);
  touch_stream(s);
  auto& slot = ws[name];
  if (!slot || slot->bytes < bytes) {
    if (slot && slot->p) RVCX_HIP(hipStreamSynchronize(s));
    slot.reset(new DevBuf());
    if (arena) {
      const size_t off = (arena_used + 255) & ~size_t(255);
      if (off + bytes > arena_bytes) {
        ws.erase(name);
        throw Error(RVCX_E_OOM, "workspace arena exhausted: " + name + " needs " + std::to_string(bytes) + " B at offset " +
                                    std::to_string(off) + " of " + std::to_string(arena_bytes));
      }
      slot->p = arena + off;
      slot->borrowed = true;
      arena_used = off + bytes;
    } else if (hipMalloc(&slot->p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      ws.erase(name);
      throw Error(RVCX_E_OOM, "workspace allocation failed: " + name + " (" + std::to_string(bytes) + " B)");
    }
    slot->bytes = bytes;
    carved += bytes;
  }
  return static_cast<T*>(slot->p);
}

// model forward passes (runtime_*.cpp)
void finalize_synth(Ctx& c);
void finalize_refinegan(Ctx& c);
long long refinegan_noise_floats(const SynthCfg& g, int B, long long T);
void refinegan_forward(Ctx& c, int B, int T, const float* z_btc, const float* mask, const float* f0, const float* g,
                       const float* eps_src, uint64_t seed, float* out, hipStream_t s);
void finalize_hubert(Ctx& c);
void finalize_rmvpe(Ctx& c);
void finalize_crepe(Ctx& c);
void finalize_fcpe(Ctx& c);
// FCPEInfer.__call__ (rvc/lib/predictors/FCPE.py:758-764) on fp32 audio, three entries to one body (runtime_fcpe.cpp
// fcpe_rows): the raw track f0 fp64 (zeros where unvoiced), salience [.][out_dims] optional; cap = the frames f0 holds.
int64_t fcpe_frames(const Ctx& c, int64_t n);  // the frames FCPEInfer gives for n samples
// the network's input alone (Wav2Mel.extract_mel): B streams of n samples -> mel [B][fcpe_frames(n)][n_mels]
int fcpe_mel(Ctx& c, const float* audio, int64_t n, int64_t ld, int B, float* mel, hipStream_t s);
// B streams of n samples: f0 [B][F], salience [B][F][out_dims]. Returns F.
int64_t fcpe_forward_b(Ctx& c, const float* audio, int64_t n, int64_t ld, int B, float thr, int mode, double* f0,
                       int64_t cap, float* sal_out, hipStream_t s);
// one utterance, then FCPEF0Predictor.post_process (:877-910) when interp_uv. Returns the frames written: F, or pad_to
int64_t fcpe_forward(Ctx& c, const float* audio, int64_t n, float thr, int mode, int interp_uv, int64_t pad_to,
                     double* f0, float* sal_out, int64_t cap, hipStream_t s);
// B inputs of nv[b] samples (host array) in one ragged pass, row b at f0 + b*ldf / sal_out + b*ld_sal*out_dims. Returns
// the longest row's frames. Equal lengths and one row are fcpe_forward_b's bits, unless `sizing` (the arena query).
int64_t fcpe_forward_v(Ctx& c, const float* audio, const int64_t* nv, int64_t ld, int B, float thr, int mode, double* f0,
                       int64_t ldf, float* sal_out, int64_t ld_sal, hipStream_t s, bool sizing = false);
// the decoders + post_process alone on salience [F][out_dims]
int64_t fcpe_decode_run(Ctx& c, const float* sal, int64_t F, float thr, int mode, int interp_uv, int64_t pad_to,
                        double* f0, hipStream_t s);
// librosa.effects.split of split_audio.process_audio (rvc/lib/tools/split_audio.py:5-27): intervals [cnt][2]
int64_t split_intervals(Ctx& c, const double* audio, int64_t n, int sr, double silence_thresh_db, int min_silence_ms,
                        int64_t* iv, int64_t cap, hipStream_t s);
// CREPE.get_f0 (rvc_mlx/lib/mlx/crepe.py:282-325) on audio [n] fp32: returns F = 1 + n/160
int64_t crepe_forward(Ctx& c, const float* audio, int64_t n, double f0_min, double f0_max, float thr, float* f0,
                      double* f0d, float* per, float* probs_out, hipStream_t s, int sem = 0,
                      const float* dither = nullptr);
int64_t hubert_forward(Ctx& c, const float* audio, int64_t n, int version, float* feats, int64_t cap,
                       hipStream_t s);
// HuBERT in three parts, so a caller can issue the encoder's last layers later on another stream:
// front end (feature convs, projection, positional conv, encoder LN), layers [l0, l1), tail (v1 projection)
constexpr int HUBERT_LAYERS = 12;
struct HubertRun {
  int B = 0, L = 0, version = 0;
  float* feats = nullptr;
  const float* mask = nullptr;  // ragged batches: [B][L], 1 on a sequence's own frames (the attention's key mask)
  // extra LDS bytes per workgroup on every conv launch of the run (ConvArgs::lds_pad): the occupancy throttle of a run
  // issued beside latency-bound work on another stream. A caller may change it between the parts.
  int lds_pad = 0;
};
HubertRun hubert_front(Ctx& c, const float* audio, int64_t n, int64_t lda, int B, int version, float* feats,
                       int64_t cap, hipStream_t s, int lds_pad = 0);
void hubert_layers(Ctx& c, const HubertRun& run, int l0, int l1, hipStream_t s);
int64_t hubert_tail(Ctx& c, const HubertRun& run, hipStream_t s);
// Work a caller wants issued beside RMVPE's BiGRU, which occupies 4 CUs per sequence (the pipeline: the rest of HuBERT
// on the aux stream). The RMVPE forwards issue it once, right after the launches of the first BiGRU group they reach;
// Ctx::ev_gate is recorded on the stream before those launches, where the hook's work may start.
using GruHook = std::function<void(hipStream_t)>;
// batched over B equal-length inputs (rows of stride lda); outputs back to back per sequence (f0 row b at f0 + b*F)
int64_t hubert_forward_b(Ctx& c, const float* audio, int64_t n, int64_t lda, int B, int version, float* feats,
                         int64_t cap, hipStream_t s);
int64_t rmvpe_forward_b(Ctx& c, const float* audio, int64_t n, int64_t lda, int B, float thred, double* f0,
                        int64_t cap, float* hidden, hipStream_t s, GruHook beside_gru = nullptr);
inline int64_t rmvpe_forward(Ctx& c, const float* audio, int64_t n, float thred, double* f0, int64_t cap, float* hidden,
                             hipStream_t s, GruHook beside_gru = nullptr) {
  return rmvpe_forward_b(c, audio, n, n, 1, thred, f0, cap, hidden, s, std::move(beside_gru));
}
// RMVPE's BiGRU recurrence on the context's hand-off buffer (runtime_fe.cpp): gi [B][T][1536] -> out [B][T][512], 16
// sequences per launch; tag_start < 0 continues the buffer's tag counters, >= 0 zeroes it and sets them (the tests).
// Tv (device, optional): sequence b runs its own Tv[b] <= T steps in rows of stride T. beside_gru (optional) is issued
// right after the BiGRU's launches.
void gru_bidir_run(Ctx& c, const float* gi, int B, int T, const float* whh_f, const float* bhh_f, const float* whh_b,
                   const float* bhh_b, float* out, long long tag_start, hipStream_t s, const int* Tv = nullptr,
                   const GruHook& beside_gru = nullptr);
// B inputs of nv[b] samples (host array) in one ragged pass: f0 row b (F_b = 1 + nv[b] / 160 frames) at f0 + b*ldf,
// its salience (optional) at hidden + b*ld_hidden*360; F_out[b] = F_b (host, optional). Returns the longest row's
// frames. Equal lengths take the pass without lengths (rmvpe_forward_b's bits), unless force_ragged (the arena query).
int64_t rmvpe_forward_v(Ctx& c, const float* audio, const int64_t* nv, int64_t lda, int B, float thred, double* f0,
                        int64_t ldf, int64_t* F_out, float* hidden, int64_t ld_hidden, hipStream_t s,
                        bool force_ragged = false);
// batched over B inputs of nv[b] samples (host array): sequence b's hubert_frames(nv[b]) rows at feats + b*ld_rows*D.
// Equal lengths run without masks, unless force_ragged.
int64_t hubert_forward_v(Ctx& c, const float* audio, const int64_t* nv, int64_t lda, int B, int version, float* feats,
                         int64_t ld_rows, int64_t* rows_out, hipStream_t s, bool force_ragged = false);
// The output samples per row a caller of the synthesizer goes on to read, [s0, s1) (s1 < 0: all of them). The HiFi-GAN
// generators (NSF and no-f0) then run on the window's frames plus their receptive field (dec_margin_frames) and write
// the window's samples, bit-identical to the full-length run, at their usual place; the samples outside it are
// unspecified. The TextEncoder and the flow run on every frame; MRF and RefineGAN ignore the window. Rows of a batch
// share it.
struct DecWindow {
  long long s0 = 0, s1 = -1;
};
// the generator's one-sided receptive field in input frames, from the loaded configuration (runtime_synth.cpp)
int dec_margin_frames(const SynthCfg& cf);
// the frames [fa, fb) of T the generator runs on for a window ([0, T) without one, or where it would drop too few)
void dec_window_frames(const SynthCfg& cf, int T, const DecWindow& win, int& fa, int& fb);
// One Synthesizer.infer call (synthesizers.py:213-243) on B rows of T frames.
struct SynthCall {
  int B = 0, T = 0;
  const float* phone = nullptr;      // [B][T][emb_dim]
  const int32_t* lengths = nullptr;  // [B]
  const int32_t* pitch = nullptr;    // [B][T], null without pitch guidance
  const float* pitchf = nullptr;
  const int32_t* sid = nullptr;  // [B]
  const float* eps_z = nullptr;  // injected noise (optional; drawn from seed otherwise)
  const float* eps_src = nullptr;
  uint64_t seed = 0;
  float* out = nullptr;  // [B][(T - head) upp]
  // optional outputs: zp_out / z_out [B][T - head][I], mp_out / logsp_out [B][T][I]
  float *zp_out = nullptr, *z_out = nullptr, *mp_out = nullptr, *logsp_out = nullptr;
  // the generator's weight-streamed convs and fused ResBlock pairs on fp16 operands (one MFMA product per step): the
  // realtime hop's opt-in (rvcx_rt_opts::gen_precision), never set by an offline entry point
  int gen_lowp = 0;
  // Synthesizer.infer's rate (synthesizers.py:230-234) as the first kept frame: the flow and the decoder run on
  // T - head frames
  int head = 0;
  DecWindow win;
  // every row has the full length T (the pipelines on rows of one length, the streaming hop): the TextEncoder's
  // attention then runs without the all-ones key mask. Same results.
  bool full_lengths = false;
};
void synth_forward(Ctx& c, const SynthCall& call, hipStream_t s);
// One generator call on z_btc [B][T][I] (time-major), mask [B][T], f0 [B][T], g [B][gin] -> out [B][T upp].
struct DecCall {
  int B = 0, T = 0;
  const float* z_btc = nullptr;
  const float* mask = nullptr;
  const float* f0 = nullptr;
  const float* g = nullptr;
  const float* eps_src = nullptr;
  uint64_t seed = 0;
  float* out = nullptr;
  int gen_lowp = 0;  // as SynthCall's
  // the NSF source and the noise convs of the multi-tap stages were computed ahead by dec_noise_prepare (same B, T,
  // f0, eps_src, seed), on a stream this one has joined since; the ConvTransposes add them as their residual
  bool noise_pre = false;
  DecWindow win;
};
void dec_forward(Ctx& c, const DecCall& call, hipStream_t s);
// the NSF harmonic source (SineGen) and every multi-tap noise conv (hifigan_nsf.py:196-199) into their own buffers:
// the synthesizer issues it on the aux stream beside the TextEncoder and flow, which leave most of the GPU idle.
// Returns false (nothing issued) for configurations without the NSF noise branch.
bool dec_noise_prepare(Ctx& c, int B, int T, const float* f0, const float* eps_src, uint64_t seed, hipStream_t s);
// the harmonic source alone, as dec_forward / dec_noise_prepare compute it (NSF SineGen or the MRF source of the loaded
// configuration): the interior of the "dec.har" rows copied to out [B][T * upp] (rvcx_dec_source, the tests)
void dec_source_rows(Ctx& c, int B, int T, const float* f0, const float* eps_src, uint64_t seed, float* out,
                     hipStream_t s);

void set_highpass(Ctx& c, const double* b, const double* a, const double* zi, int order);
void set_highpass_sos(Ctx& c, const double* sos, int nsec);
// filtfilt + reflect pad of one utterance with whichever high-pass form is configured
void highpass_pad(Ctx& c, const double* audio, int64_t n, int64_t t_pad, double* pad64, float* pad32, hipStream_t s);
int hubert_version_for(const Ctx& c);
// feats_pre (optional): HuBERT rows of this chunk computed ahead (e.g. on the aux stream), L_pre rows
// trim: samples per side of the output the caller drops (the pipeline's t_pad_tgt, or 0 while the window is off): for
// trim > 0 the generator gets the kept window (DecWindow), and the trimmed samples of out are then unspecified
int64_t vc_forward(Ctx& c, const float* audio, int64_t n, const int32_t* pitch, const float* pitchf,
                   int64_t pitch_len, int sid, float protect, double index_rate, const float* eps_z,
                   const float* eps_src, uint64_t seed, float* out, int64_t cap, hipStream_t s,
                   const float* feats_pre = nullptr, int64_t L_pre = 0, int64_t trim = 0);
// streaming (runtime_stream.cpp)
struct RtState;
RtState* rt_create(Ctx& c, const rvcx_rt_desc& d);
void rt_destroy(RtState* s);
void rt_geometry(const RtState& s, int64_t* g);
void rt_reset(Ctx& c, RtState& s, hipStream_t st);
void rt_reset_stream(Ctx& c, RtState& s, int stream_index, hipStream_t st);
int rt_streams(const RtState& s);
// the voice of slot b (-1: every slot); refusals as rvcx_rt_set_voice documents them, no slot changed then
void rt_set_voice(Ctx& c, RtState& s, int b, int voice);
void rt_get_voices(const RtState& s, int32_t* out);
// opts [B], one per slot; active [B] (0 = the slot sits this hop out) or null = every slot active
void rt_process(Ctx& c, RtState& s, const float* in48, const int32_t* sids, const rvcx_rt_opts* opts,
                const uint8_t* active, const float* eps_z, const float* eps_src, uint64_t seed, float* out48,
                float* vol_out, int* offs_out, hipStream_t st);
// The noise gate of the realtime path (TorchGate's stationary mode; kernels in spectral_gate.hip) over x [B][n] ->
// y [B][n], samples [256 (n / 256), n) zeros; d_strength [B] on the device, negative = the row is copied through;
// mask_out (optional) [B][513][1 + n / 256]. spectral_gate_check throws RVCX_E_SHAPE for n < 2048 or a sampling rate
// whose smoothing filter is empty, and launches nothing.
void spectral_gate_check(int64_t n, int sr);
void spectral_gate_run(Ctx& c, const float* x, int B, int64_t n, int64_t ldx, int sr, const float* d_strength,
                       float* y, int64_t ldy, uint8_t* mask_out, hipStream_t st);
// the noise gate of one slot (b = -1: every slot) on or off; throws RVCX_E_INVALID and changes nothing for a strength
// outside [0, 1] or a geometry the gate cannot serve (runtime_stream.cpp)
void rt_set_clean(Ctx& c, RtState& s, int b, int clean_audio, double clean_strength);
// the last hop's model rows [B_act][frames * upp] before (gated = 0) or after (1) the noise gate -> dst (rows ld apart)
void rt_model_rows(const RtState& s, int gated, float* dst, int64_t ld, hipStream_t st);
// index (index_ivf.cpp)
struct ParsedIvf {  // a validated faiss IndexIVFFlat image on the host (lists in list order)
  int d = 0, nprobe = 1;
  long long nlist = 0, ntotal = 0;
  std::vector<float> cent, vecs;
  std::vector<long long> off, ids;
  std::vector<int> slot;  // id -> slot
  bool sparse_sizes = false;  // the file's list sizes were "sprs" pairs, not a "full" vector
};
ParsedIvf parse_ivf(const uint8_t* bytes, int64_t nbytes);  // host only; throws Error(RVCX_E_INVALID)
void index_load(Ctx& c, const uint8_t* bytes, int64_t nbytes);
void index_search(Ctx& c, const float* x, int64_t n, int k, float* dist, int64_t* ids, hipStream_t s);
void index_retrieve(Ctx& c, const float* feats, int64_t L, int d, double index_rate, float* out, hipStream_t s);
// the blend for n_seq sequences of feats / out [.][L][d] in one search: rows off.. of sequence seqs[i] at
// rate[seqs[i]] / one_minus_rate[seqs[i]] (device arrays); no other row of out is written
void index_retrieve_rows(Ctx& c, const float* feats, int64_t L, int64_t off, int d, int n_seq, const int* seqs,
                         const float* rate, const float* one_minus_rate, float* out, hipStream_t s);
void index_reconstruct_n(Ctx& c, int64_t i0, int64_t ni, float* out, hipStream_t s);
// index build and write (index_build.cpp): faiss train + add over x [n][d] (extract_index.py:58-68); the result
// replaces the loaded index once the build has succeeded
void index_build(Ctx& c, const float* x, int64_t n, int d, int64_t nlist, const rvcx_index_build_opts& o,
                 hipStream_t s);
void index_centroids(Ctx& c, float* out, hipStream_t s);  // the loaded index's centroids [nlist][d]
// faiss.write_index of the loaded index (extract_index.py:70) -> the byte count; bytes == null: the count alone
int64_t index_save(Ctx& c, void* bytes, int64_t cap);
// the k-means kernels on their own (rvcx_test.h)
void kmeans_assign_run(Ctx& c, const float* x, int64_t n, int d, const float* cent, int64_t nlist, int32_t* assign,
                       float* dist, hipStream_t s);
void kmeans_update_run(Ctx& c, const float* x, int64_t n, int d, const int32_t* assign, int64_t nlist, float* cent,
                       int64_t* sizes, hipStream_t s);
// sizing (here and in pipeline_forward_rows): the call is pipeline_workspace_bytes' measurement and takes the
// worst-case routes, so that the pool it carves holds any real call of that size -- a long input the chunk plan with
// the longest possible chunk, a batch the ragged form for equal rows too, and the generator no output window
int64_t pipeline_forward_ex(Ctx& c, const double* audio, int64_t n, const rvcx_pipeline_opts& o,
                            const float* eps_z, const float* eps_src, uint64_t seed, float* out, int64_t cap,
                            double* f0_out, hipStream_t s, bool sizing);
int64_t pipeline_forward_batch(Ctx& c, const double* audio, int64_t n, int64_t lda, int B, const rvcx_pipeline_opts& o,
                               const int32_t* sids, const float* eps_z, const float* eps_src, uint64_t seed,
                               float* out, int64_t ldo, double* f0_out, float* hidden_out, hipStream_t s);
// The batched pipeline. B utterances of nv[b] samples (host array), rows of stride lda: out row b n_out[b] samples,
// f0_out row b at stride ldf; hidden_out (RMVPE's salience) only for rows of one length. pipeline_forward_batch above
// is this with every nv[b] = n. voices (host [B], optional): the voice of each row, rows of one voice contiguous
// (rvcx_pipeline_batch_voices); null = every row on the current voice.
void pipeline_forward_rows(Ctx& c, const double* audio, const int64_t* nv, int64_t lda, int B,
                           const rvcx_pipeline_opts& o, const int32_t* sids, const float* eps_z, const float* eps_src,
                           uint64_t seed, float* out, int64_t ldo, int64_t* n_out, double* f0_out, int64_t ldf,
                           float* hidden_out, hipStream_t s, bool sizing, const int32_t* voices = nullptr);
// rvcx_workspace_bytes: the pool a pipeline call of B utterances of n samples under o takes, measured by running it on
// zero audio from an empty pool (B = 1 pipeline_forward_ex, B > 1 pipeline_forward_rows in its sizing form); a caller
// arena is detached meanwhile and the pool is released again before it returns
int64_t pipeline_workspace_bytes(Ctx& c, int B, int64_t n, const rvcx_pipeline_opts& o, hipStream_t s);
rvcx_pipeline_opts default_pipeline_opts();
// the reference predictors' voicing thresholds (FCPE's: rvc/realtime/pipeline.py:155); a positive one of the caller wins
constexpr float RMVPE_THRESHOLD = 0.03f, FCPE_THRESHOLD = 0.006f;
inline float or_default(float v, float d) { return v > 0 ? v : d; }
inline float rmvpe_threshold(const rvcx_pipeline_opts& o) { return or_default(o.rmvpe_threshold, RMVPE_THRESHOLD); }
inline float fcpe_threshold(const rvcx_pipeline_opts& o) { return or_default(o.fcpe_threshold, FCPE_THRESHOLD); }
// whether the loaded FCPE gives the pipelines' pitch frames (160 samples at 16 kHz): RVCX_OK, RVCX_E_STATE without
// finalized FCPE weights, RVCX_E_SHAPE for another rate or hop; and the refusal of f0 method "fcpe" that goes with it
inline int fcpe_pitch_frames(const Ctx& c) {
  return !c.ready[RVCX_MODEL_FCPE] ? RVCX_E_STATE : c.fcfg.sr == 16000 && c.fcfg.hop == 160 ? RVCX_OK : RVCX_E_SHAPE;
}
inline void require_fcpe_pitch_frames(const Ctx& c, const std::string& who) {
  const int e = fcpe_pitch_frames(c);
  if (e == RVCX_E_STATE) throw Error(e, who + ": f0_method fcpe but no FCPE weights finalized");
  if (e != RVCX_OK) throw Error(e, who + ": the FCPE model must run at 16 kHz with hop_size 160");
}
int proposed_key(const std::vector<double>& f0, double threshold);
int64_t hubert_frames(int64_t n);  // HuBERT output rows for n samples (0 when too short)
void set_i32(int32_t* p, int32_t v, hipStream_t s);
void set_i32_once(Ctx& c, const std::string& name, int32_t* p, int32_t v, hipStream_t s);
// Overlap of independent stages: fork_aux returns the aux stream, ordered after everything queued on s so
// far (or s itself when overlap is off: kernel timing on, or RVCX_NO_OVERLAP=1); join_aux makes s wait for
// everything queued on the aux stream so far.
hipStream_t fork_aux(Ctx& c, hipStream_t s);
// whether launch_conv's plan runs this 1-D contraction on the weight-streamed fp16 or the weight-stationary kernel
// without split-K (the kernels whose epilogue takes the fused NSF noise conv, ConvArgs::nz_*)
bool conv_routes_wsb16(Ctx& c, const ConvArgs& a);
void join_aux(Ctx& c, hipStream_t s, hipStream_t ax);
// launch one implicit-GEMM conv (1-D or 2-D) as conv_plan routes it, with optional event timing; flops = algorithmic
// FLOPs (runtime_conv.cpp)
void launch_conv(Ctx& c, const ConvArgs& a_in, bool two_d, hipStream_t s, double flops = -1.0);
// launch_conv for the kernel-level test entries: the plan under `force`, refused with RVCX_E_SHAPE before any launch
// where the forced family does not admit the form, the family is not expect_kind (>= 0) or the combine's epilogues get
// no split; a fresh weight image built per call. Returns the plan it ran.
ConvPlan launch_conv_test(Ctx& c, const ConvArgs& a_in, bool two_d, bool static_weight, const ConvForce& force,
                          int expect_kind, const char* who, hipStream_t s);
// one fused ResBlock pair (resblock_fused.hip) with optional event timing (counted with the conv family)
void launch_rb_pair(Ctx& c, const RbPairArgs& a, hipStream_t s);
inline void check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw Error(RVCX_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace rvcx
