// Streaming voice conversion (config C5): a group of B concurrent streams of one buffer geometry,
// converted together per hop on the caller's stream.
//
// Reference: rvc/realtime/core.py -- VoiceChanger (:329-484), Realtime.realloc (:165-216),
// Realtime.inference (:217-326) -- and rvc/realtime/pipeline.py Realtime_Pipeline.get_f0 (:122-212) /
// voice_conversion (:214-334) / _retrieve_speaker_embeddings (:336-352). The MLX port of this path is
// not functional, so the PyTorch semantics are followed.
//
// Per hop, all on device: 48k -> 16k resample (torchaudio sinc kernel), circular audio/convert buffers
// and the RMS gate, RMVPE or FCPE f0 (rvcx_rt_desc::f0_method; one batched forward over the B convert buffers either
// way) + realtime quantisation into the circular pitch buffers, HuBERT (+ repeated
// last frame), optional index retrieval from skip_head // 2, x2 upsample + protect, one batched
// Synthesizer.infer over the B streams, clip, [volume envelope], [noise gate], * sqrt(vol), [tgt -> 48k resample],
// SOLA offset search + crossfade. The host only plans (and syncs once per hop for proposed_pitch).
//
// Every option is per slot (one rvcx_rt_opts each), and a slot may sit a hop out. The networks run on the B_act active
// slots compacted to rows 0..B_act-1; the state kernels (rt_ingest, rt_pitch, rt_up2, rt_sola) map rows to slots with
// the device slot map (stream.hip). The per-row options, the synthesizer's lengths / sids and the slot map travel in
// one upload per hop (RowPlan). With every slot active the map is the identity and is not passed.
#include <cmath>
#include <cstring>

#include "model_build.h"

namespace rvcx {

namespace {

// torchaudio's Resample(..., dtype=torch.float32) with its defaults (sinc_interp_hann, width 6, rolloff 0.99;
// core.py:99-108)
SincKernel sinc_kernel(int orig_freq, int new_freq) {
  return sinc_resample_kernel(orig_freq, new_freq, 6.0, 0.99, SINC_HANN, 0.0);
}

// One hop's per-row plan as it lies in device memory (every array sized for the group's B slots, the first B_act
// entries valid unless noted): uploaded once per hop, `factor` again after the proposed-pitch sync.
struct RowPlan {
  size_t factor, strength, protect, rate, one_minus_rate, rms, autotune, use_protect, seqs, meta, slot2row, row2slot;
  size_t clean;
  size_t bytes;
  explicit RowPlan(int B) {
    size_t o = 0;
    auto take = [&](size_t elem, size_t n) {
      const size_t at = o;
      o += elem * n * (size_t)B;
      return at;
    };
    factor = take(sizeof(double), 1);    // 2^(key / 12), 1 under autotune
    strength = take(sizeof(double), 1);  // autotune strength
    protect = take(sizeof(float), 1);
    rate = take(sizeof(float), 1);  // (float)index_rate and (float)(1 - index_rate)
    one_minus_rate = take(sizeof(float), 1);
    rms = take(sizeof(float), 1);  // volume_envelope
    autotune = take(sizeof(int), 1);
    use_protect = take(sizeof(int), 1);
    seqs = take(sizeof(int), 1);       // the rows that retrieve (n_ret entries)
    meta = take(sizeof(int32_t), 2);   // lengths [B_act] at 0, sids [B_act] at B
    slot2row = take(sizeof(int), 1);   // [B], -1 = idle
    row2slot = take(sizeof(int), 1);
    clean = take(sizeof(float), 1);    // clean_strength where clean_audio is set, else -1 (the gate copies the row)
    bytes = o;
  }
};

template <class T>
void dev_alloc(DevBuf& b, size_t count) {
  const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  if (hipMalloc(&b.p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    throw Error(RVCX_E_OOM, "stream state allocation failed");
  }
  b.bytes = bytes;
  RVCX_HIP(hipMemset(b.p, 0, bytes));
}

}  // namespace

struct RtState {
  int B = 0;
  int block48 = 0, cross48 = 0, extra48 = 0, sola48 = 0;
  int block16 = 0, cross16 = 0, sola16 = 0, extra16 = 0;
  int conv16 = 0, feat = 0, skip_head = 0, return_length = 0, silence_front = 0;
  int n16 = 0;      // resampled input length per hop (ceil(block48 / 3))
  int abuf_n = 0, pbuf_n = 0;
  double sensitivity = 1.0;
  int tgt_sr = 48000;
  SincKernel kin, kout;
  bool out_identity = true;
  DevBuf d_kin, d_kout, abuf[2], cbuf[2], pbuf[2], fbuf[2], sola, fade_in, offs, vol, volsq, gate, rows;
  int cur = 0;
  int f0_method = 0;  // 0 RMVPE, 1 FCPE (rvcx_rt_desc)
  float fcpe_thr = FCPE_THRESHOLD;
  // the last hop's model rows [last_rows][last_n] as the noise gate read them and as it left them (the same buffer on
  // a hop without a cleaning stream): pool buffers of the context, valid until its next call (rvcx_rt_model_rows)
  const float *last_model = nullptr, *last_gated = nullptr;
  int last_rows = 0;
  int64_t last_n = 0;
  // per slot: the noise gate's strength (rt_set_clean), negative = the slot does not clean. A setting of the slot like
  // its sid, not hop state: rt_reset / rt_reset_stream leave it.
  std::vector<float> clean;
  // per slot: its voice (rt_set_voice), a setting like the sid; geom: what every voice of the group shares, taken from
  // the voice the group was created on
  std::vector<int> voice;
  VoiceGeom geom;
};

// TorchGate's filter half widths as Python's double arithmetic gives them: n_grad_freq = int(500 / (sr / (n_fft / 2))),
// n_grad_time = int(50 / ((hop / sr) * 1000)) bins / frames
static void sg_filter_sizes(int sr, int& nf, int& nt) {
  nf = (int)(500.0 / ((double)sr / 512.0));
  nt = (int)(50.0 / ((256.0 / (double)sr) * 1000.0));
}

void spectral_gate_check(int64_t n, int sr) {
  if (n < 2 * SG_NFFT) throw Error(RVCX_E_SHAPE, "spectral_gate: needs at least 2048 samples per row");
  int nf = 0, nt = 0;
  if (sr > 0) sg_filter_sizes(sr, nf, nt);
  if (sr <= 0 || nf < 1 || nt < 1 || nf > SG_MAX_HALF || nt > SG_MAX_HALF)
    throw Error(RVCX_E_SHAPE, "spectral_gate: the sampling rate gives an empty smoothing filter");
}

void spectral_gate_run(Ctx& c, const float* x, int B, int64_t n, int64_t ldx, int sr, const float* d_strength,
                       float* y, int64_t ldy, uint8_t* mask_out, hipStream_t st) {
  spectral_gate_check(n, sr);
  int nf = 0, nt = 0;
  sg_filter_sizes(sr, nf, nt);
  if (!c.dev.count("sg.tables")) {  // the twiddles and the window, once per context
    std::vector<float> tab(SG_TAB_FLOATS);
    sg_tables(tab.data());
    c.alloc_weight("sg.tables", tab);
  }
  const float* tab = static_cast<const float*>(c.dev["sg.tables"]->p);
  const size_t cells = (size_t)B * (size_t)sg_frames(n) * SG_BINS;
  float* X = c.buf<float>("sg.X", 2 * cells, st);
  float* db = c.buf<float>("sg.db", cells, st);
  uint8_t* mask = c.buf<uint8_t>("sg.mask", cells, st);
  float* frames = c.buf<float>("sg.frames", (size_t)B * (size_t)sg_frames(n) * SG_NFFT, st);
  check(spectral_gate(x, ldx, n, d_strength, nf, nt, tab, X, db, mask, frames, y, ldy, mask_out, B, st),
        "spectral_gate");
}

// Realtime(..., clean_audio, clean_strength) of one slot (core.py:86-94), or of every slot (b = -1). Refused, with no
// slot changed: a strength outside [0, 1] (TorchGate asserts it), a model row shorter than the gate's 2048 samples, and
// a geometry in which a sample SOLA reads (a[off + j], off <= sola48, j < block48 + cross48) would come from the tail
// [256 * (n_model / 256), n_model) that the gate writes as zeros -- for tgt_sr != 48000 through the output resampler,
// whose sample j reads the model's samples up to (j / nw) * orig + width + orig - 1 (k_rt_resample).
void rt_set_clean(Ctx& c, RtState& s, int b, int clean_audio, double clean_strength) {
  if (b < -1 || b >= s.B) throw Error(RVCX_E_INVALID, "stream: stream_index out of range");
  float v = -1.f;
  if (clean_audio) {
    if (!(clean_strength >= 0.0 && clean_strength <= 1.0))
      throw Error(RVCX_E_INVALID, "stream: clean_strength must lie in [0, 1]");
    const int64_t n_model = (int64_t)s.feat * s.geom.upp;
    if (n_model < 2 * SG_NFFT) throw Error(RVCX_E_INVALID, "stream: clean_audio needs a model row of 2048 samples");
    try {
      spectral_gate_check(n_model, s.tgt_sr);
    } catch (const Error& e) {
      throw Error(RVCX_E_INVALID, std::string("stream: clean_audio: ") + e.what());
    }
    const int64_t last48 = (int64_t)s.sola48 + s.block48 + s.cross48 - 1;
    const int64_t last_model =
        s.out_identity ? last48 : (last48 / s.kout.nw) * s.kout.orig + s.kout.width + s.kout.orig - 1;
    if (last_model >= sg_n_out(n_model))
      throw Error(RVCX_E_INVALID, "stream: clean_audio: SOLA would read the gate's zeroed tail in this geometry");
    v = (float)clean_strength;
  }
  for (int i = 0; i < s.B; ++i)
    if (b < 0 || i == b) s.clean[(size_t)i] = v;
}

void rt_model_rows(const RtState& s, int gated, float* dst, int64_t ld, hipStream_t st) {
  if (!s.last_model || s.last_rows < 1) throw Error(RVCX_E_STATE, "rt_model_rows: no hop with an active stream yet");
  if (!dst || ld < s.last_n) throw Error(RVCX_E_INVALID, "rt_model_rows: null destination or ld below the row length");
  RVCX_HIP(hipMemcpy2DAsync(dst, sizeof(float) * (size_t)ld, gated ? s.last_gated : s.last_model,
                            sizeof(float) * (size_t)s.last_n, sizeof(float) * (size_t)s.last_n, (size_t)s.last_rows,
                            hipMemcpyDeviceToDevice, st));
}

RtState* rt_create(Ctx& c, const rvcx_rt_desc& d) {
  if (!c.ready[RVCX_MODEL_SYNTH] || !c.ready[RVCX_MODEL_HUBERT])
    throw Error(RVCX_E_STATE, "stream: synth and hubert must be finalized");
  if (d.f0_method < 0 || d.f0_method > 1) throw Error(RVCX_E_INVALID, "stream: f0_method must be 0 (rmvpe) or 1 (fcpe)");
  if (c.scfg.f0 && d.f0_method == 0 && !c.ready[RVCX_MODEL_RMVPE])
    throw Error(RVCX_E_STATE, "stream: f0_method rmvpe but no RMVPE weights finalized");
  if (c.scfg.f0 && d.f0_method == 1) require_fcpe_pitch_frames(c, "stream");  // as the pipeline's f0_method 3
  if (d.n_streams < 1 || d.n_streams > 4096) throw Error(RVCX_E_INVALID, "stream: n_streams out of range");
  if (d.read_chunk_size < 1) throw Error(RVCX_E_INVALID, "stream: read_chunk_size < 1");
  auto r = std::make_unique<RtState>();
  RtState& s = *r;
  const double AUDIO_SR = 48000.0, SR = 16000.0;
  const int window = 160;
  s.B = d.n_streams;
  s.clean.assign((size_t)s.B, -1.f);
  s.voice.assign((size_t)s.B, c.cur_voice);
  s.geom = voice_geom(c.scfg);
  s.f0_method = d.f0_method;
  s.fcpe_thr = or_default(d.fcpe_threshold, FCPE_THRESHOLD);
  // VoiceChanger.__init__ (core.py:351-354)
  s.block48 = d.read_chunk_size * 128;
  s.cross48 = (int)(d.cross_fade_overlap_size * AUDIO_SR);
  s.extra48 = (int)(d.extra_convert_size * AUDIO_SR);
  s.sola48 = 48000 / 100;
  // Realtime.realloc (core.py:172-199)
  s.block16 = (int)((double)s.block48 / AUDIO_SR * SR);
  s.cross16 = (int)((double)s.cross48 / AUDIO_SR * SR);
  s.sola16 = (int)((double)s.sola48 / AUDIO_SR * SR);
  s.extra16 = (int)((double)s.extra48 / AUDIO_SR * SR);
  int conv = s.block16 + s.sola16 + s.extra16 + s.cross16;
  if (conv % window) conv += window - conv % window;
  s.conv16 = conv;
  s.feat = conv / window;
  s.skip_head = s.extra16 / window;
  s.return_length = s.feat - s.skip_head;
  s.silence_front = 0;  // Realtime.__init__ sets 0, so realloc keeps 0 (core.py:57, :200-202)
  s.abuf_n = s.block16 + s.cross16;
  s.pbuf_n = s.feat + 1;
  s.sensitivity = std::pow(10.0, d.silent_threshold / 20.0);
  s.tgt_sr = c.scfg.sr;
  s.kin = sinc_kernel(48000, 16000);
  s.n16 = (int)std::ceil((double)s.kin.nw * s.block48 / s.kin.orig);
  if (s.n16 > s.abuf_n || s.n16 > s.conv16) throw Error(RVCX_E_INVALID, "stream: block larger than its buffers");
  s.out_identity = s.tgt_sr == 48000;
  if (!s.out_identity) s.kout = sinc_kernel(s.tgt_sr, 48000);
  const int upp = c.scfg.upp();
  const int64_t n_model = (int64_t)s.feat * upp;
  const int64_t n48 = s.out_identity ? n_model : (int64_t)std::ceil((double)s.kout.nw * n_model / s.kout.orig);
  if (n48 < (int64_t)s.sola48 + s.block48 + s.cross48)
    throw Error(RVCX_E_INVALID, "stream: model output shorter than sola search + block + crossfade");
  const int64_t L = hubert_frames(s.conv16);
  if (L < 1 || 2 * L + 1 < s.feat) throw Error(RVCX_E_INVALID, "stream: convert buffer too short for HuBERT");
  if (s.skip_head / 2 >= L) throw Error(RVCX_E_INVALID, "stream: skip_head beyond the feature frames");
  RVCX_HIP(hipSetDevice(c.device));
  dev_alloc<float>(s.d_kin, s.kin.k.size());
  RVCX_HIP(hipMemcpy(s.d_kin.p, s.kin.k.data(), s.kin.k.size() * sizeof(float), hipMemcpyHostToDevice));
  if (!s.out_identity) {
    dev_alloc<float>(s.d_kout, s.kout.k.size());
    RVCX_HIP(hipMemcpy(s.d_kout.p, s.kout.k.data(), s.kout.k.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  for (int i = 0; i < 2; ++i) {
    dev_alloc<float>(s.abuf[i], (size_t)s.B * s.abuf_n);
    dev_alloc<float>(s.cbuf[i], (size_t)s.B * s.conv16);
    dev_alloc<int>(s.pbuf[i], (size_t)s.B * s.pbuf_n);
    dev_alloc<float>(s.fbuf[i], (size_t)s.B * s.pbuf_n);
  }
  dev_alloc<float>(s.sola, (size_t)s.B * s.cross48);
  // fade_in = sin(0.5*pi*linspace(0, 1, cf))**2 in float32 (core.py:376-396; torch linspace's
  // two-sided formula)
  std::vector<float> fi((size_t)std::max(1, s.cross48));
  const int cf = s.cross48;
  if (cf == 1) {
    fi[0] = 0.f;
  } else if (cf > 1) {
    const float step = 1.0f / (float)(cf - 1);
    const int half = cf / 2;
    const float hp = (float)(0.5 * M_PI);
    for (int i = 0; i < cf; ++i) {
      const float x = i < half ? step * (float)i : 1.0f - step * (float)(cf - i - 1);
      const float v = std::sin(hp * x);
      fi[i] = v * v;
    }
  }
  dev_alloc<float>(s.fade_in, fi.size());
  RVCX_HIP(hipMemcpy(s.fade_in.p, fi.data(), fi.size() * sizeof(float), hipMemcpyHostToDevice));
  dev_alloc<int>(s.offs, s.B);
  dev_alloc<float>(s.vol, s.B);
  dev_alloc<float>(s.volsq, s.B);
  dev_alloc<int>(s.gate, s.B);
  dev_alloc<char>(s.rows, RowPlan(s.B).bytes);
  return r.release();
}

void rt_destroy(RtState* s) { delete s; }

void rt_geometry(const RtState& s, int64_t* g) {
  const int64_t v[12] = {s.B,        s.block48,       s.block16,       s.conv16,     s.feat,    s.skip_head,
                         s.return_length, s.cross48, s.sola48, s.extra48, s.n16, s.silence_front};
  std::memcpy(g, v, sizeof(v));
}

void rt_reset(Ctx& c, RtState& s, hipStream_t st) {
  (void)c;
  for (int i = 0; i < 2; ++i) {
    RVCX_HIP(hipMemsetAsync(s.abuf[i].p, 0, s.abuf[i].bytes, st));
    RVCX_HIP(hipMemsetAsync(s.cbuf[i].p, 0, s.cbuf[i].bytes, st));
    RVCX_HIP(hipMemsetAsync(s.pbuf[i].p, 0, s.pbuf[i].bytes, st));
    RVCX_HIP(hipMemsetAsync(s.fbuf[i].p, 0, s.fbuf[i].bytes, st));
  }
  RVCX_HIP(hipMemsetAsync(s.sola.p, 0, s.sola.bytes, st));
  s.cur = 0;
}

int rt_streams(const RtState& s) { return s.B; }

namespace {
// a voice of the bank without selecting it: its configuration, readiness and index wherever they are held
struct VoiceRef {
  const SynthCfg* cfg = nullptr;
  bool ready = false;
  const IvfIndex* ivf = nullptr;
};
VoiceRef voice_ref(const Ctx& c, int id) {
  if (id == c.cur_voice) return {&c.scfg, c.ready[RVCX_MODEL_SYNTH], c.ivf.get()};
  const Voice& v = c.voices.at(id);
  return {&v.scfg, v.ready, v.ivf.get()};
}
}  // namespace

void rt_set_voice(Ctx& c, RtState& s, int b, int voice) {
  if (b < -1 || b >= s.B) throw Error(RVCX_E_INVALID, "stream: stream_index out of range");
  if (!c.has_voice(voice)) throw Error(RVCX_E_INVALID, "stream: voice " + std::to_string(voice) + " does not exist (or was freed)");
  const VoiceRef v = voice_ref(c, voice);
  if (!v.ready) throw Error(RVCX_E_STATE, "stream: voice " + std::to_string(voice) + " is not finalized");
  if (!(voice_geom(*v.cfg) == s.geom))
    throw Error(RVCX_E_SHAPE, "stream: voice " + std::to_string(voice) + " differs from the group's geometry voice in sr, "
                              "upsample product, text_enc_hidden_dim, inter_channels, no_f0 or vocoder");
  for (int i = 0; i < s.B; ++i)
    if (b < 0 || i == b) s.voice[(size_t)i] = voice;
}

void rt_get_voices(const RtState& s, int32_t* out) {
  for (int i = 0; i < s.B; ++i) out[i] = s.voice[(size_t)i];
}

// One slot back to its created state. Both halves of each ping-pong pair are cleared, so the slot reads zeros
// whichever half is current; no other slot's bytes are touched.
void rt_reset_stream(Ctx& c, RtState& s, int b, hipStream_t st) {
  (void)c;
  if (b < 0 || b >= s.B) throw Error(RVCX_E_INVALID, "stream: stream_index out of range");
  auto zero = [&](DevBuf& d, size_t row_bytes) {
    RVCX_HIP(hipMemsetAsync(static_cast<char*>(d.p) + (size_t)b * row_bytes, 0, row_bytes, st));
  };
  for (int i = 0; i < 2; ++i) {
    zero(s.abuf[i], sizeof(float) * s.abuf_n);
    zero(s.cbuf[i], sizeof(float) * s.conv16);
    zero(s.pbuf[i], sizeof(int) * s.pbuf_n);
    zero(s.fbuf[i], sizeof(float) * s.pbuf_n);
  }
  if (s.cross48 > 0) zero(s.sola, sizeof(float) * s.cross48);
}

void rt_process(Ctx& c, RtState& s, const float* in48, const int32_t* sids, const rvcx_rt_opts* opts,
                const uint8_t* active, const float* eps_z, const float* eps_src, uint64_t seed, float* out48,
                float* vol_out, int* offs_out, hipStream_t st) {
  const int B = s.B, E = s.geom.emb_dim, upp = s.geom.upp, I = s.geom.I;
  // The compact rows are the active slots ordered by voice: the voice groups by their lowest active slot, the rows of a
  // group by slot. With one voice in use that is slot order.
  struct Group {
    int voice, r0, n, k0, n_ret;  // rows [r0, r0 + n); its retrieving rows are entries [k0, k0 + n_ret) of the plan's seqs
  };
  std::vector<Group> groups;
  std::vector<int> slot2row(B, -1), row2slot;
  for (int b = 0; b < B; ++b) {
    if ((active && !active[b]) || slot2row[b] >= 0) continue;
    Group g{s.voice[(size_t)b], (int)row2slot.size(), 0, 0, 0};
    for (int q = b; q < B; ++q)
      if ((!active || active[q]) && s.voice[(size_t)q] == g.voice) {
        slot2row[q] = (int)row2slot.size();
        row2slot.push_back(q);
      }
    g.n = (int)row2slot.size() - g.r0;
    groups.push_back(g);
  }
  const int Ba = (int)row2slot.size();
  bool all = Ba == B;  // the row map is the identity (every slot active, in slot order): it is not passed then
  for (int r = 0; r < Ba && all; ++r) all = row2slot[r] == r;
  const bool guided = s.geom.f0 != 0;  // no get_f0, pitch or protect without pitch guidance (pipeline.py:242-293)
  for (const Group& g : groups) {  // a slot's voice may have been freed or re-finalized since rt_set_voice
    if (!c.has_voice(g.voice))
      throw Error(RVCX_E_STATE, "stream: voice " + std::to_string(g.voice) + " of an active slot was freed");
    const VoiceRef v = voice_ref(c, g.voice);
    if (!v.ready || !(voice_geom(*v.cfg) == s.geom))
      throw Error(RVCX_E_STATE, "stream: voice " + std::to_string(g.voice) + " of an active slot is not finalized, or "
                                "no longer has the group's geometry");
  }
  int n_ret = 0, n_prop = 0;
  bool any_tune = false, any_rms = false, any_clean = false;
  const int64_t n_model = (int64_t)s.feat * upp;
  for (int r = 0; r < Ba; ++r) {
    const int b = row2slot[r];
    const rvcx_rt_opts& o = opts[b];
    const VoiceRef v = voice_ref(c, s.voice[(size_t)b]);
    if (sids[b] < 0 || sids[b] >= v.cfg->n_spk) throw Error(RVCX_E_INVALID, "stream: sid out of range");
    if (o.index_rate > 0 && !v.ivf) throw Error(RVCX_E_STATE, "stream: index_rate > 0 but no feature index loaded");
    if (o.gen_precision < 0 || o.gen_precision > 1)
      throw Error(RVCX_E_INVALID, "stream: gen_precision must be 0 (fp32) or 1 (fp16 generator)");
    if (o.gen_precision != opts[row2slot[0]].gen_precision)
      throw Error(RVCX_E_INVALID, "stream: the active streams of one hop must agree on gen_precision");
    if (o.index_rate > 0 && v.ivf->view.d != E) throw Error(RVCX_E_SHAPE, "stream: index dimension mismatch");
    n_ret += o.index_rate > 0 ? 1 : 0;
    any_tune |= o.f0_autotune != 0;
    n_prop += (!o.f0_autotune && o.proposed_pitch) ? 1 : 0;
    any_rms |= o.volume_envelope != 1.0;
    any_clean |= s.clean[b] >= 0.f;  // validated when it was set (rt_set_clean)
  }
  if ((!all || groups.size() > 1) && eps_src && s.geom.vocoder != 0)
    throw Error(RVCX_E_INVALID, "stream: injected source noise with idle slots or several voices needs the HiFi-GAN-NSF "
                                "noise layout");
  if (Ba == 0) {  // nobody took part: zero outputs, no state touched
    RVCX_HIP(hipMemsetAsync(out48, 0, sizeof(float) * (size_t)B * s.block48, st));
    if (vol_out) RVCX_HIP(hipMemsetAsync(vol_out, 0, sizeof(float) * B, st));
    if (offs_out) RVCX_HIP(hipMemsetAsync(offs_out, 0, sizeof(int) * B, st));
    return;
  }
  const int gen_precision = opts[row2slot[0]].gen_precision;
  const int T = s.feat;
  // the hop's plan: per-row options, synthesizer lengths / sids, slot map -- one upload
  const RowPlan P(B);
  std::vector<char> plan(P.bytes, 0);
  auto at = [&](size_t off) { return plan.data() + off; };
  double* h_fac = reinterpret_cast<double*>(at(P.factor));
  double* h_str = reinterpret_cast<double*>(at(P.strength));
  float* h_prot = reinterpret_cast<float*>(at(P.protect));
  float* h_rate = reinterpret_cast<float*>(at(P.rate));
  float* h_omr = reinterpret_cast<float*>(at(P.one_minus_rate));
  float* h_rms = reinterpret_cast<float*>(at(P.rms));
  int* h_tune = reinterpret_cast<int*>(at(P.autotune));
  int* h_usep = reinterpret_cast<int*>(at(P.use_protect));
  int* h_seqs = reinterpret_cast<int*>(at(P.seqs));
  int32_t* h_meta = reinterpret_cast<int32_t*>(at(P.meta));
  std::memcpy(at(P.slot2row), slot2row.data(), sizeof(int) * B);
  std::memcpy(at(P.row2slot), row2slot.data(), sizeof(int) * Ba);
  for (Group& g : groups) {
    for (int r = 0; r < g.r0; ++r) g.k0 += opts[row2slot[r]].index_rate > 0 ? 1 : 0;
    for (int r = g.r0; r < g.r0 + g.n; ++r) g.n_ret += opts[row2slot[r]].index_rate > 0 ? 1 : 0;
  }
  for (int r = 0, k = 0; r < Ba; ++r) {
    const int b = row2slot[r];
    const rvcx_rt_opts& o = opts[b];
    // autotune replaces the shift (pipeline.py:157-158); a proposed key is added after the sync below
    h_fac[r] = o.f0_autotune ? 1.0 : std::pow(2.0, o.f0_up_key / 12.0);
    h_str[r] = o.f0_autotune_strength;
    h_tune[r] = o.f0_autotune ? 1 : 0;
    h_prot[r] = o.protect;
    h_usep[r] = (guided && o.protect < 0.5f) ? 1 : 0;
    // torch: npy * index_rate + (1 - index_rate) * feats, python scalars cast to float32 (1 - r in double)
    h_rate[r] = (float)o.index_rate;
    h_omr[r] = (float)(1.0 - o.index_rate);
    if (o.index_rate > 0) h_seqs[k++] = r;
    h_rms[r] = (float)o.volume_envelope;
    reinterpret_cast<float*>(at(P.clean))[r] = s.clean[b];
    h_meta[r] = T;
    h_meta[B + r] = sids[b];
  }
  char* dplan = static_cast<char*>(s.rows.p);
  // A copy from pageable memory holds the host until it is staged. With idle slots the first kernel reads the slot
  // map, so the plan goes first; with every slot active nothing reads it before the f0 network is queued, and the
  // copy is issued behind that, where the device has work to do meanwhile.
  auto upload_plan = [&] {
    RVCX_HIP(hipMemcpyAsync(dplan, plan.data(), P.bytes, hipMemcpyHostToDevice, st));
  };
  if (!all) upload_plan();
  const double* d_fac = reinterpret_cast<const double*>(dplan + P.factor);
  const int32_t* dmeta = reinterpret_cast<const int32_t*>(dplan + P.meta);
  const int* d_s2r = all ? nullptr : reinterpret_cast<const int*>(dplan + P.slot2row);
  const int* d_r2s = all ? nullptr : reinterpret_cast<const int*>(dplan + P.row2slot);
  const int nxt = 1 - s.cur;
  // 1. input resample 48k -> 16k, circular buffers, RMS gate (core.py:227-267); idle slots carry their state over
  float* in16 = c.buf<float>("rt.in16", (size_t)B * s.n16, st);
  check(rt_resample(in48, s.block48, s.block48, static_cast<const float*>(s.d_kin.p), s.kin.K, s.kin.width, s.kin.orig,
                    s.kin.nw, in16, s.n16, s.n16, nullptr, d_s2r, B, st),
        "rt_resample_in");
  float* conv_rows = all ? nullptr : c.buf<float>("rt.conv", (size_t)Ba * s.conv16, st);
  check(rt_ingest(in16, s.n16, static_cast<float*>(s.abuf[s.cur].p), static_cast<float*>(s.abuf[nxt].p), s.abuf_n,
                  static_cast<float*>(s.cbuf[s.cur].p), static_cast<float*>(s.cbuf[nxt].p), s.conv16, s.sensitivity,
                  static_cast<float*>(s.vol.p), static_cast<float*>(s.volsq.p), static_cast<int*>(s.gate.p), d_s2r,
                  conv_rows, B, st),
        "rt_ingest");
  // the B_act convert buffers the networks see: the state itself when every slot is active
  const float* conv = all ? static_cast<const float*>(s.cbuf[nxt].p) : conv_rows;
  // 2. f0 on the convert buffer (pipeline.py:233-245 -> get_f0 :122-212)
  const int nf = s.conv16 - s.silence_front;
  const int F = 1 + nf / 160;
  if (F > s.pbuf_n) throw Error(RVCX_E_SHAPE, "stream: f0 track longer than the pitch buffer");
  double* f0 = c.buf<double>("rt.f0", (size_t)Ba * F, st);
  const int64_t L = hubert_frames(s.conv16);
  float* feats = c.buf<float>("rt.feats", (size_t)Ba * L * E, st);
  hipStream_t ax = fork_aux(c, st);  // batched HuBERT beside the batched f0 network (pipeline.py:233-254)
  hubert_forward_b(c, conv, s.conv16, s.conv16, Ba, E == 256 ? 1 : 2, feats, L, ax);
  if (guided) {
  if (s.f0_method == 1) {  // the raw local_argmax track (pipeline.py:147-155), F = nf / 160 + 1 frames as RMVPE's
    if (fcpe_pitch_frames(c) != RVCX_OK)
      throw Error(RVCX_E_STATE, "stream: the FCPE model this group was created with has been replaced");
    if (fcpe_forward_b(c, conv + s.silence_front, nf, s.conv16, Ba, s.fcpe_thr, 0, f0, F, nullptr, st) != F)
      throw Error(RVCX_E_SHAPE, "stream: FCPE frame count differs from the pitch track's");
  } else {
    rmvpe_forward_b(c, conv + s.silence_front, nf, s.conv16, Ba, RMVPE_THRESHOLD, f0, F, nullptr, st);
  }
  }
  if (all) upload_plan();
  if (guided) {
  if (any_tune)  // rows without autotune keep their f0 bits
    check(f0_autotune_rows(f0, F, reinterpret_cast<const double*>(dplan + P.strength),
                           reinterpret_cast<const int*>(dplan + P.autotune), Ba, st),
          "f0_autotune");
  if (n_prop > 0) {  // the proposed key is a host median (pipeline.py:159-183): only the asking rows come back
    std::vector<double> h((size_t)Ba * F);
    for (int r = 0; r < Ba;) {
      auto asks = [&](int q) { return !opts[row2slot[q]].f0_autotune && opts[row2slot[q]].proposed_pitch; };
      if (!asks(r)) {
        ++r;
        continue;
      }
      int e = r + 1;
      while (e < Ba && asks(e)) ++e;  // one copy per run of neighbouring rows
      RVCX_HIP(hipMemcpyAsync(h.data() + (size_t)r * F, f0 + (size_t)r * F, sizeof(double) * (size_t)(e - r) * F,
                              hipMemcpyDeviceToHost, st));
      r = e;
    }
    RVCX_HIP(hipStreamSynchronize(st));
    c.check_device_status();
    for (int r = 0; r < Ba; ++r) {
      const rvcx_rt_opts& o = opts[row2slot[r]];
      if (o.f0_autotune || !o.proposed_pitch) continue;
      std::vector<double> one(h.begin() + (size_t)r * F, h.begin() + (size_t)(r + 1) * F);
      h_fac[r] = std::pow(2.0, (o.f0_up_key + proposed_key(one, o.proposed_pitch_threshold)) / 12.0);
    }
    RVCX_HIP(hipMemcpyAsync(dplan + P.factor, h_fac, sizeof(double) * Ba, hipMemcpyHostToDevice, st));
  }
  check(rt_pitch(f0, F, d_fac, static_cast<const int*>(s.pbuf[s.cur].p), static_cast<int*>(s.pbuf[nxt].p),
                 static_cast<const float*>(s.fbuf[s.cur].p), static_cast<float*>(s.fbuf[nxt].p), s.pbuf_n, d_s2r, B,
                 st),
        "rt_pitch");
  } else if (!all) {  // no pitch track to write, but an idle slot's (unused) pitch state still follows the flip
    RVCX_HIP(hipMemcpyAsync(s.pbuf[nxt].p, s.pbuf[s.cur].p, s.pbuf[nxt].bytes, hipMemcpyDeviceToDevice, st));
    RVCX_HIP(hipMemcpyAsync(s.fbuf[nxt].p, s.fbuf[s.cur].p, s.fbuf[nxt].bytes, hipMemcpyDeviceToDevice, st));
  }
  // 3. HuBERT over the B_act convert buffers (pipeline.py:248-254), rows [B_act][L][E]
  join_aux(c, st, ax);
  // 4. index retrieval of rows skip_head // 2 .. (pipeline.py:264-268, :336-352): one search over every row that
  // retrieves, each blended at its own rate; the rest of the features is a plain copy
  // -- per voice, against that voice's index
  VoiceScope restore(c);  // the groups select their voices; the context's current voice comes back, on an error too
  const float* fx = feats;
  if (n_ret > 0) {
    float* fr = c.buf<float>("rt.feats_idx", (size_t)Ba * L * E, st);
    RVCX_HIP(hipMemcpyAsync(fr, feats, sizeof(float) * (size_t)Ba * L * E, hipMemcpyDeviceToDevice, st));
    for (const Group& g : groups) {
      if (g.n_ret == 0) continue;
      c.select_voice(g.voice);
      index_retrieve_rows(c, feats, L, s.skip_head / 2, E, g.n_ret, reinterpret_cast<const int*>(dplan + P.seqs) + g.k0,
                          reinterpret_cast<const float*>(dplan + P.rate),
                          reinterpret_cast<const float*>(dplan + P.one_minus_rate), fr, st);
    }
    fx = fr;
  }
  // 5. x2 upsample [:p_len] + protect; pitch tails (pipeline.py:270-293)
  float* phone = c.buf<float>("rt.phone", (size_t)Ba * T * E, st);
  int32_t* pitch = c.buf<int32_t>("rt.pitch", (size_t)Ba * T, st);
  float* pitchf = c.buf<float>("rt.pitchf", (size_t)Ba * T, st);
  const double formant = std::ceil(s.return_length * 1.0);
  const float pscale = (float)(formant / (double)s.return_length);
  check(rt_up2(fx, feats, (int)L, E, phone, T, static_cast<const float*>(s.fbuf[nxt].p), s.pbuf_n, pscale,
               reinterpret_cast<const float*>(dplan + P.protect), reinterpret_cast<const int*>(dplan + P.use_protect),
               pitch, static_cast<const int*>(s.pbuf[nxt].p), pitchf, d_r2s, Ba, st),
        "rt_up2");
  // 6. one batched Synthesizer.infer per voice over its rows (pipeline.py:295-297), clip (:93). Injected noise is
  // indexed by slot, so unless the row map is the identity the active slots' rows are gathered first.
  if (!all && eps_z) {
    float* ez = c.buf<float>("rt.eps_z", (size_t)Ba * I * T, st);
    check(gather_rows(eps_z, I * T, d_r2s, ez, Ba, I * T, st), "rt_eps_z");
    eps_z = ez;
  }
  if (!all && eps_src) {
    float* es = c.buf<float>("rt.eps_src", (size_t)Ba * n_model, st);
    check(gather_rows(eps_src, (int)n_model, d_r2s, es, Ba, (int)n_model, st), "rt_eps_src");
    eps_src = es;
  }
  float* model = c.buf<float>("rt.model", (size_t)Ba * n_model, st);
  const int64_t n_need = std::min<int64_t>(n_model, (int64_t)s.sola48 + s.block48 + s.cross48);
  int64_t n_clip = n_model;
  for (const Group& g : groups) {
    c.select_voice(g.voice);
    const size_t r0 = (size_t)g.r0;
    SynthCall syn;
    syn.B = g.n, syn.T = T;
    syn.phone = phone + r0 * T * E, syn.lengths = dmeta + r0, syn.sid = dmeta + B + r0;
    if (guided) syn.pitch = pitch + r0 * T, syn.pitchf = pitchf + r0 * T;
    // the NSF layout is one row of noise per batch row (checked above for several groups); drawn noise is keyed by the
    // row within the call, so the groups after the first draw under seeds of their own
    syn.eps_z = eps_z ? eps_z + r0 * I * T : nullptr, syn.eps_src = eps_src ? eps_src + r0 * n_model : nullptr;
    syn.seed = seed + 0x9E3779B97F4A7C15ull * (uint64_t)g.r0;
    syn.out = model + r0 * n_model;
    syn.gen_lowp = gen_precision;
    syn.full_lengths = true;  // every stream's hop is T frames (meta above)
    // k_rt_sola reads a[off + j], off <= sola48, j < block48 + cross48: the only reader of the model's output where
    // it is neither resampled nor RMS-adjusted nor gated (the gate's statistics run over the whole row), so the
    // generator runs on that window alone
    if (s.out_identity && !any_rms && !any_clean && c.dec_window) syn.win = {0, n_need};
    synth_forward(c, syn, st);
    if (syn.win.s1 >= 0) n_clip = n_need;
  }
  check(rt_clip(model, n_model, (int)n_clip, Ba, st), "rt_clip");
  if (any_rms) {  // pipeline.py:299-307 (source = the 16 kHz convert buffer); rows at exactly 1 are skipped
    const int n1 = rms_frame_count(s.conv16, 16000), n2 = rms_frame_count(n_model, s.tgt_sr);
    float* ws = c.buf<float>("rt.rms", (size_t)Ba * (n1 + n2), st);
    check(change_rms(conv, s.conv16, (int)s.conv16, s.conv16, 16000, model, n_model, (int)n_model, n_model, s.tgt_sr,
                     1.f, reinterpret_cast<const float*>(dplan + P.rms), ws, st, Ba),
          "change_rms");
  }
  // the noise gate on the rows that ask for it (pipeline.py:326-327: after the volume envelope, before * sqrt(vol)),
  // out of place; the other rows are copied through
  s.last_model = s.last_gated = model;
  s.last_rows = Ba;
  s.last_n = n_model;
  if (any_clean) {
    float* gated = c.buf<float>("rt.model_clean", (size_t)Ba * n_model, st);
    spectral_gate_run(c, model, Ba, n_model, n_model, s.tgt_sr, reinterpret_cast<const float*>(dplan + P.clean), gated,
                      n_model, nullptr, st);
    model = gated;
    s.last_gated = gated;
  }
  // 7. * sqrt(vol) [-> 48 kHz], SOLA crossfade (core.py:324, :404-451)
  const float* a48 = model;
  int64_t lda = n_model;
  const float* scale = static_cast<const float*>(s.volsq.p);
  if (!s.out_identity) {
    const int64_t n48 = (int64_t)std::ceil((double)s.kout.nw * n_model / s.kout.orig);
    float* r48 = c.buf<float>("rt.model48", (size_t)Ba * n48, st);
    check(rt_resample(model, n_model, (int)n_model, static_cast<const float*>(s.d_kout.p), s.kout.K, s.kout.width,
                      s.kout.orig, s.kout.nw, r48, n48, (int)n48, scale, nullptr, Ba, st),
          "rt_resample_out");
    a48 = r48;
    lda = n48;
    scale = nullptr;
  }
  check(rt_sola(a48, lda, scale, static_cast<const int*>(s.gate.p), static_cast<float*>(s.sola.p), s.cross48,
                s.sola48, static_cast<const float*>(s.fade_in.p), out48, s.block48,
                offs_out ? offs_out : static_cast<int*>(s.offs.p), d_s2r, B, st),
        "rt_sola");
  if (vol_out) RVCX_HIP(hipMemcpyAsync(vol_out, s.vol.p, sizeof(float) * B, hipMemcpyDeviceToDevice, st));
  s.cur = nxt;
}

}  // namespace rvcx
