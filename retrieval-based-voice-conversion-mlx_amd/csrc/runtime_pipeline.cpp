// Whole-utterance pipeline on device: Pipeline.pipeline (rvc/infer/pipeline.py:390-558;
// rvc_mlx/infer/pipeline_mlx.py:263-373) = filtfilt -> reflect pad -> RMVPE -> get_f0 adjustments ->
// [split at quiet points when longer than t_max] -> per chunk HuBERT -> x2 upsample + protect ->
// Synthesizer.infer -> trim -> concatenate -> change_rms -> peak normalise.
//
// Everything that touches samples runs as HIP kernels on the caller's stream. The host only plans:
// it reads back the split points (long inputs) and, for proposed_pitch, the f0 track whose median
// sets the key offset (pipeline.py:250-277) -- both are a few KB and need one stream sync each.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rows.h"

namespace rvcx {

void set_highpass(Ctx& c, const double* b, const double* a, const double* zi, int order) {
  if (order < 1 || order > IIR_MAXO) throw Error(RVCX_E_INVALID, "highpass order out of range");
  if (!(a[0] != 0.0)) throw Error(RVCX_E_INVALID, "highpass a[0] == 0");
  c.hp_order = order;
  c.hp_sos = SosPlan();  // a new (b, a) filter drops any section form set for the previous one
  c.hp_b.assign(b, b + order + 1);
  c.hp_a.assign(a, a + order + 1);
  c.hp_zi.assign(zi, zi + order);
  const double a0 = a[0];
  for (auto& v : c.hp_b) v /= a0;
  for (auto& v : c.hp_a) v /= a0;
}

// SOS plan (iir_scan.hip): per section the DF2T biquad and its steady state for a unit pass input (scipy
// filtfilt's zi * x0: the whole cascade at rest on the constant x0, DC gains of the preceding sections
// included); for the cascade as one system A^(L 2^s) for the carry scan and the rows C A^k of the chunk fix-up.
void set_highpass_sos(Ctx& c, const double* sos, int nsec) {
  if (nsec < 1 || nsec > IIR_MAXO) throw Error(RVCX_E_INVALID, "highpass: bad section count");
  SosPlan p;
  p.nsec = nsec;
  if (nsec > 4) throw Error(RVCX_E_INVALID, "highpass: more than 4 sections");
  // per section: b0 b1 b2 a1 a2, then its two steady-state values
  struct Sec {
    double t[5], w[2];
  };
  std::vector<Sec> sec(nsec);
  double gain = 1.0;  // DC gain of the sections before j
  for (int j = 0; j < nsec; ++j) {
    const double* q = sos + 6 * j;
    if (!(q[3] != 0.0)) throw Error(RVCX_E_INVALID, "highpass: section a0 == 0");
    const double b0 = q[0] / q[3], b1 = q[1] / q[3], b2 = q[2] / q[3], a1 = q[4] / q[3], a2 = q[5] / q[3];
    double* t = sec[j].t;
    t[0] = b0, t[1] = b1, t[2] = b2, t[3] = a1, t[4] = a2;
    // steady state z = (I - A)^-1 B u with A = [[-a1, 1], [-a2, 0]], B = [b1 - a1 b0, b2 - a2 b0], u = gain
    const double B0 = b1 - a1 * b0, B1 = b2 - a2 * b0;
    const double det = (1.0 + a1) * 1.0 + a2;  // det(I - A) = (1 + a1) * 1 - (-1) * (a2)
    if (!(std::fabs(det) > 1e-300)) throw Error(RVCX_E_INVALID, "highpass: section has a pole at z = 1");
    // (I - A) = [[1 + a1, -1], [a2, 1]] -> inverse = [[1, 1], [-a2, 1 + a1]] / det
    sec[j].w[0] = (B0 + B1) / det * gain;
    sec[j].w[1] = (-a2 * B0 + (1.0 + a1) * B1) / det * gain;
    gain *= (b0 + b1 + b2) / (1.0 + a1 + a2);
  }
  // the cascade as ONE system of NS = 2 nsec states (iir_scan.hip casc_filtfilt_pad): its A and C by stepping the
  // cascade from unit states with zero input, the steady state w = the per-section states above, A^(L 2^s) and
  // the rows C A^k of the chunk fix-up
  const int NS = 2 * nsec, L = p.casc_L;
  std::vector<double> tab(48 + 64 * 12 + 8 * (size_t)L, 0.0);
  double* ct = tab.data();
  std::vector<double> A((size_t)NS * NS), C(NS);
  auto step = [&](const double* z, double x, double* zo) {
    double u = x;
    for (int j = 0; j < nsec; ++j) {
      const double* t = sec[j].t;
      const double y = t[0] * u + z[2 * j];
      zo[2 * j] = t[1] * u - t[3] * y + z[2 * j + 1];
      zo[2 * j + 1] = t[2] * u - t[4] * y;
      u = y;
    }
    return u;
  };
  for (int i = 0; i < NS; ++i) {
    std::vector<double> z(NS, 0.0), zo(NS, 0.0);
    z[i] = 1.0;
    C[i] = step(z.data(), 0.0, zo.data());
    for (int r = 0; r < NS; ++r) A[(size_t)r * NS + i] = zo[r];
  }
  for (int j = 0; j < nsec; ++j) {
    for (int q = 0; q < 5; ++q) ct[5 * j + q] = sec[j].t[q];
    ct[40 + 2 * j] = sec[j].w[0];
    ct[40 + 2 * j + 1] = sec[j].w[1];
  }
  auto mul = [&](const std::vector<double>& X, const std::vector<double>& Y) {
    std::vector<double> Z((size_t)NS * NS, 0.0);
    for (int r = 0; r < NS; ++r)
      for (int q = 0; q < NS; ++q)
        for (int k = 0; k < NS; ++k) Z[(size_t)r * NS + q] += X[(size_t)r * NS + k] * Y[(size_t)k * NS + q];
    return Z;
  };
  std::vector<double> M((size_t)NS * NS, 0.0);
  for (int i = 0; i < NS; ++i) M[(size_t)i * NS + i] = 1.0;
  std::vector<double> row(C);  // C A^k
  for (int k = 0; k < L; ++k) {
    for (int i = 0; i < NS; ++i) ct[48 + 64 * 12 + 8 * k + i] = row[i];
    std::vector<double> nr(NS, 0.0);
    for (int q = 0; q < NS; ++q)
      for (int i = 0; i < NS; ++i) nr[q] += row[i] * A[(size_t)i * NS + q];
    row = nr;
    M = mul(A, M);  // A^(k + 1)
  }
  for (int sidx = 0; sidx < 12; ++sidx) {  // pow[s] = A^(L 2^s), NS x NS in an 8 x 8 block
    for (int r = 0; r < NS; ++r)
      for (int q = 0; q < NS; ++q) ct[48 + 64 * sidx + 8 * r + q] = M[(size_t)r * NS + q];
    M = mul(M, M);
  }
  RVCX_HIP(hipSetDevice(c.device));
  c.hp_sos_buf.reset();
  const size_t bytes = tab.size() * sizeof(double);
  if (hipMalloc(&c.hp_sos_buf.p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    throw Error(RVCX_E_OOM, "highpass: device allocation failed");
  }
  c.hp_sos_buf.bytes = bytes;
  RVCX_HIP(hipMemcpy(c.hp_sos_buf.p, tab.data(), bytes, hipMemcpyHostToDevice));
  p.casc = static_cast<const double*>(c.hp_sos_buf.p);
  c.hp_sos = p;
}

void highpass_pad(Ctx& c, const double* audio, int64_t n, int64_t t_pad, double* pad64, float* pad32, hipStream_t s) {
  if (c.hp_order == 0) throw Error(RVCX_E_STATE, "pipeline: high-pass filter not configured");
  if (c.hp_sos.nsec > 0) {
    double* ws = c.buf<double>("pl.sosws", filtfilt_sos_ws_doubles(n, c.hp_order), s);
    check(filtfilt_sos_pad(c.hp_sos, c.hp_order, audio, n, t_pad, ws, pad64, pad32, s), "filtfilt_sos");
    return;
  }
  double* ws = c.buf<double>("pl.iirws", filtfilt_ws_doubles(n, c.hp_order), s);
  check(filtfilt_pad(audio, n, c.hp_b.data(), c.hp_a.data(), c.hp_zi.data(), c.hp_order, t_pad, ws, pad64, pad32,
                     s),
        "filtfilt_pad");
}

int hubert_version_for(const Ctx& c) { return c.scfg.emb_dim == 256 ? 1 : 2; }

int64_t vc_forward(Ctx& c, const float* audio, int64_t n, const int32_t* pitch, const float* pitchf,
                   int64_t pitch_len, int sid, float protect, double index_rate, const float* eps_z,
                   const float* eps_src, uint64_t seed, float* out, int64_t cap, hipStream_t s,
                   const float* feats_pre, int64_t L_pre, int64_t trim) {
  if (sid < 0 || sid >= c.scfg.n_spk) throw Error(RVCX_E_INVALID, "sid out of range");
  const int E = c.scfg.emb_dim;
  const float* feats = feats_pre;
  int64_t L = L_pre;
  if (!feats) {
    const int64_t cap_rows = n / 320 + 8;  // HuBERT frames for n samples (upper bound n/320)
    float* fb = c.buf<float>("vc.feats", (size_t)cap_rows * E, s);
    L = hubert_forward(c, audio, n, hubert_version_for(c), fb, cap_rows, s);
    feats = fb;
  }
  const int T = (int)std::min<int64_t>(n / 160, 2 * L);
  if (T <= 0) throw Error(RVCX_E_SHAPE, "voice_conversion: input shorter than one frame");
  if (c.scfg.f0 && (!pitch || !pitchf)) throw Error(RVCX_E_INVALID, "voice_conversion: pitch-guided model needs pitch");
  if (!c.scfg.f0) pitch = nullptr, pitchf = nullptr;  // pitch_guidance False: no protect, no pitch (pipeline.py:324-365)
  if (pitch && T > pitch_len) throw Error(RVCX_E_SHAPE, "voice_conversion: pitch track shorter than the features");
  const int upp = c.scfg.upp();
  if ((int64_t)T * upp > cap)
    throw Error(RVCX_E_CAPACITY, "voice_conversion: output needs " + std::to_string((int64_t)T * upp) + " samples");
  // speaker-embedding retrieval on the raw features (pipeline.py:338-342); feats0 stays raw for protect
  const float* fx = feats;
  if (index_rate > 0 && c.ivf) {
    float* fr = c.buf<float>("vc.feats_idx", (size_t)L * E, s);
    index_retrieve(c, feats, L, E, index_rate, fr, s);
    fx = fr;
  }
  float* phone = c.buf<float>("vc.phone", (size_t)T * E, s);
  check(upsample2_protect(fx, feats, (int)L, (int)L, E, phone, T, T, protect < 0.5f ? pitchf : nullptr, 0, protect, s),
        "upsample");
  int32_t* lens = c.buf<int32_t>("vc.len", 4, s);
  set_i32_once(c, "vc.len.T", lens, T, s);
  set_i32_once(c, "vc.len.sid", lens + 1, sid, s);
  SynthCall syn;
  syn.B = 1, syn.T = T;
  syn.phone = phone, syn.lengths = lens, syn.pitch = pitch, syn.pitchf = pitchf, syn.sid = lens + 1;
  syn.eps_z = eps_z, syn.eps_src = eps_src, syn.seed = seed;
  syn.out = out;
  syn.full_lengths = true;
  if (trim > 0) syn.win = {trim, (long long)T * upp - trim};
  synth_forward(c, syn, s);
  return (int64_t)T * upp;
}

// key offset of proposed_pitch (pipeline.py:250-277): median of the voiced-interpolated track
int proposed_key(const std::vector<double>& f0, double threshold) {
  std::vector<int64_t> valid;
  for (size_t i = 0; i < f0.size(); ++i)
    if (f0[i] > 0) valid.push_back((int64_t)i);
  if (valid.size() < 2) return 0;
  // np.interp(arange(F), valid, f0[valid]): clamps outside [valid[0], valid[-1]]
  std::vector<double> v(f0.size());
  size_t k = 0;
  for (size_t i = 0; i < f0.size(); ++i) {
    const int64_t x = (int64_t)i;
    if (x <= valid.front()) {
      v[i] = f0[valid.front()];
    } else if (x >= valid.back()) {
      v[i] = f0[valid.back()];
    } else {
      while (valid[k + 1] < x) ++k;
      const double x0 = (double)valid[k], x1 = (double)valid[k + 1];
      const double y0 = f0[valid[k]], y1 = f0[valid[k + 1]];
      v[i] = (x == valid[k + 1]) ? y1 : y0 + (y1 - y0) * ((double)x - x0) / (x1 - x0);
    }
  }
  std::sort(v.begin(), v.end());
  const size_t m = v.size();
  const double med = (m & 1) ? v[m / 2] : 0.5 * (v[m / 2 - 1] + v[m / 2]);
  if (!(med > 0)) return 0;
  const double key = std::nearbyint(12.0 * std::log2(threshold / med));  // np.round: half to even
  return (int)std::max(-12.0, std::min(12.0, key));
}

// f0_method of rvcx_pipeline_opts against the loaded models
static void check_f0_method(const Ctx& c, const rvcx_pipeline_opts& o) {
  if (o.f0_method < 0 || o.f0_method > 5)
    throw Error(RVCX_E_INVALID,
                "pipeline: f0_method must be 0 (rmvpe), 1 (crepe, MLX), 2 (crepe, rvc/), 3 (fcpe), 4 (rmvpe, ragged) or "
                "5 (fcpe, ragged)");
  if (!c.scfg.f0) return;
  if ((o.f0_method == 1 || o.f0_method == 2) && !c.ready[RVCX_MODEL_CREPE])
    throw Error(RVCX_E_STATE, "pipeline: f0_method crepe but no CREPE weights finalized");
  if (o.f0_method == 3 || o.f0_method == 5) require_fcpe_pitch_frames(c, "pipeline");
}

// the option checks of both pipeline forms, for utterances of n samples
static void check_pipeline_opts(const Ctx& c, const rvcx_pipeline_opts& o, int64_t n) {
  if (c.hp_order == 0) throw Error(RVCX_E_STATE, "pipeline: high-pass filter not configured");
  if (o.t_pad < 0 || o.t_pad_tgt < 0 || o.t_pad >= n) throw Error(RVCX_E_INVALID, "pipeline: bad t_pad");
  check_f0_method(c, o);
  if (o.index_rate > 0 && !c.ivf) throw Error(RVCX_E_STATE, "pipeline: index_rate > 0 but no feature index loaded");
  if (o.version != 0 && o.version != hubert_version_for(c))
    throw Error(RVCX_E_INVALID, "pipeline: version does not match the synthesizer's embedding width");
}

// One row's f0 [F] over its padded input of m samples for the methods that run per row. CREPE: PitchExtractor.extract
// (rvc_mlx/lib/mlx/pitch_extractors.py:155-156) with PipelineMLX's f0_min 50 / f0_max 1100 and CREPE.get_f0's threshold
// 0.1; f0_method 2: rvc/'s CREPE.get_f0 (pipeline.py:223-234), viterbi decode without its dither. FCPE (f0_method 3):
// FCPE.get_f0 (rvc/lib/predictors/f0.py:71-89), the raw local_argmax track. f0f names CREPE's fp32 work buffer.
static void f0_row(Ctx& c, const rvcx_pipeline_opts& o, const float* audio, int64_t m, double* f0, int64_t F,
                   const char* f0f, hipStream_t s) {
  if (o.f0_method == 3) {
    fcpe_forward(c, audio, m, fcpe_threshold(o), 0, 0, 0, f0, nullptr, F, s);
  } else {
    crepe_forward(c, audio, m, 50.0, 1100.0, 0.1f, c.buf<float>(f0f, (size_t)F, s), f0, nullptr, nullptr, s,
                  o.f0_method == 2 ? 1 : 0);
  }
}

// get_f0's adjustments (pipeline.py:248-291) of f0 in place, then the coarse / fine pitch per row, for rows of Fv[b]
// frames at stride ld (f0, pitch, pitchf; f0_out rows at stride ldf): autotune (one launch when the rows lie back to
// back), or the proposed-pitch key of each row (one device -> host copy and sync), then f0_post with the row's shift
static void pitch_from_f0(Ctx& c, const rvcx_pipeline_opts& o, double* f0, int B, const int64_t* Fv, int64_t ld,
                          int32_t* pitch, float* pitchf, double* f0_out, int64_t ldf, hipStream_t s) {
  std::vector<double> shift(B, o.pitch);
  if (o.f0_autotune) {
    const int skip = o.mlx_semantics ? 1 : 0;
    if (std::all_of(Fv, Fv + B, [&](int64_t F) { return F == ld; })) {
      check(f0_autotune(f0, (int)(B * ld), o.f0_autotune_strength, skip, s), "f0_autotune");
    } else {
      for (int b = 0; b < B; ++b)
        check(f0_autotune(f0 + (size_t)b * ld, (int)Fv[b], o.f0_autotune_strength, skip, s), "f0_autotune");
    }
    if (!o.mlx_semantics) std::fill(shift.begin(), shift.end(), 0.0);  // rvc/: autotune replaces the shift (:248-279)
  } else if (o.proposed_pitch) {
    std::vector<double> h((size_t)B * ld);
    RVCX_HIP(hipMemcpyAsync(h.data(), f0, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
    RVCX_HIP(hipStreamSynchronize(s));
    c.check_device_status();
    for (int b = 0; b < B; ++b) {
      std::vector<double> one(h.begin() + (size_t)b * ld, h.begin() + (size_t)b * ld + Fv[b]);
      shift[b] = o.pitch + proposed_key(one, o.proposed_pitch_threshold);
    }
  }
  for (int b = 0; b < B; ++b)
    check(f0_post(f0 + (size_t)b * ld, (int)Fv[b], std::pow(2.0, shift[b] / 12.0), pitch + (size_t)b * ld,
                  pitchf + (size_t)b * ld, f0_out ? f0_out + (size_t)b * ldf : nullptr, s),
          "f0_post");
}

int64_t pipeline_forward_ex(Ctx& c, const double* audio, int64_t n, const rvcx_pipeline_opts& opts,
                            const float* eps_z, const float* eps_src, uint64_t seed, float* out, int64_t cap,
                            double* f0_out, hipStream_t s, bool sizing) {
  check_pipeline_opts(c, opts, n);
  rvcx_pipeline_opts o = opts;
  if (o.f0_method == 4) o.f0_method = 0;  // one utterance: the ragged RMVPE pass is the single-row one
  if (o.f0_method == 5) o.f0_method = 3;  // and the ragged FCPE pass likewise
  if (o.index_rate > 0 && c.ivf->view.d != c.scfg.emb_dim)
    throw Error(RVCX_E_SHAPE, "pipeline: feature index dimension does not match the model's feature width");
  const int64_t W = 160;  // Pipeline.window
  const int64_t m = n + 2 * o.t_pad;
  // 1. zero-phase high-pass, reflect pad t_pad (pipeline.py:439, :459); fp64 copy kept for the split
  //    search and the RMS envelope, fp32 copy feeds the models (torch.from_numpy(...).float()).
  float* pad32 = c.buf<float>("pl.pad32", (size_t)m, s);
  double* pad64 = c.buf<double>("pl.pad64", (size_t)m, s);
  highpass_pad(c, audio, n, o.t_pad, pad64, pad32, s);
  const double* filtered = pad64 + o.t_pad;
  // 2. split points for inputs longer than t_max (pipeline.py:440-452)
  std::vector<int64_t> opt_ts;
  if (o.t_max > 0 && n + W > o.t_max && o.t_center > 0) {
    if (o.t_query <= 0 || o.t_query > o.t_center) throw Error(RVCX_E_INVALID, "pipeline: bad t_query/t_center");
    const int nts = n > o.t_center ? (int)((n - 1 - o.t_center) / o.t_center + 1) : 0;
    double* sum = c.buf<double>("pl.winsum", (size_t)n, s);
    long long* dts = c.buf<long long>("pl.ts", (size_t)std::max(1, nts), s);
    check(split_points(filtered, n, (int)W, o.t_center, o.t_query, sum, dts, nts, s), "split_points");
    opt_ts.resize(nts);
    if (nts > 0 && sizing) {
      // rvcx_workspace_bytes: the plan whose longest chunk is the longest any audio can give (each split point lies
      // in [k t_center - t_query, k t_center + t_query]): a middle chunk from the lowest split to the highest next one
      // (or, with one split, the first chunk up to its highest split); the rest centred
      for (int k = 0; k < nts; ++k) opt_ts[k] = (int64_t)(k + 1) * o.t_center;
      if (nts == 1) opt_ts[0] += o.t_query;
      else opt_ts[0] -= o.t_query, opt_ts[1] += o.t_query;
      for (auto& t : opt_ts) t = std::max<int64_t>(0, std::min<int64_t>(t, n - 1));
    } else if (nts > 0) {
      RVCX_HIP(hipMemcpyAsync(opt_ts.data(), dts, sizeof(long long) * nts, hipMemcpyDeviceToHost, s));
      RVCX_HIP(hipStreamSynchronize(s));
      c.check_device_status();
    }
  }
  // 3. chunk plan (pipeline.py:486-512): [a0, a1) samples and [f_lo, f_hi) pitch frames per chunk
  struct Chunk {
    int64_t a0, a1, f_lo, f_hi;
  };
  std::vector<Chunk> chunks;
  {
    const int64_t t_pad2 = 2 * o.t_pad;
    int64_t st = 0, t = 0;
    bool have_t = false;
    for (int64_t t_raw : opt_ts) {
      t = t_raw / W * W;
      chunks.push_back({st, std::min(m, t + t_pad2 + W), st / W, (t + t_pad2) / W});
      st = t;
      have_t = true;
    }
    chunks.push_back(have_t ? Chunk{t, m, t / W, m / W} : Chunk{0, m, 0, m / W});
  }
  // 4. HuBERT of every chunk on the aux stream, beside RMVPE on the caller's stream (they only share
  //    the padded input); the chunk loop waits for it before the upsample. Kernel timing (rvcx_profile)
  //    and RVCX_NO_OVERLAP=1 keep it on the caller's stream so per-kernel durations are not shared.
  const int E = c.scfg.emb_dim;
  std::vector<float*> cfeats(chunks.size());
  std::vector<int64_t> cL(chunks.size());
  //    The encoder's last layers are issued only when RMVPE reaches its BiGRU (which holds 4 CUs for ~2 ms):
  //    the U-Net then shares the GPU with less of HuBERT and the rest of HuBERT fills the BiGRU's idle CUs.
  hipStream_t ax = fork_aux(c, s);
  static const int gate_layer = [] {
    const char* e = rvcx_knob("RVCX_HUBERT_GATE");  // first layer issued beside the BiGRU (12: none)
    // A/B on MI355X (BiGRU launched first), round 2: 2 21.84 ms, 3 21.87, 4 21.96, 1 22.03, 0 22.12, 6 22.30; round 4 (same
    // box, 4 runs each, profiles/r04q_ab_hubert_gate.txt): 0 13.39 ms, 1 13.45, 2 13.53 -- with the fp16-split U-Net
    // and HuBERT the whole encoder fits beside the BiGRU, and the U-Net then shares the GPU with the front alone
    const int v = e ? std::atoi(e) : 0;
    return v < 0 ? 0 : (v > HUBERT_LAYERS ? HUBERT_LAYERS : v);
  }();
  // without pitch guidance there is no RMVPE (pipeline.py:461-472 skipped): HuBERT runs in one piece
  const bool guided = c.scfg.f0;
  const int split = (ax != s && guided) ? gate_layer : HUBERT_LAYERS;
  std::vector<HubertRun> hruns(chunks.size());
  // chunks are processed longest first: every later chunk fits the shared work buffers the first one grew, so a
  // call regrows nothing past its first chunk (a caller-sized arena, rvcx_workspace_bytes, holds any split plan);
  // the per-chunk noise offsets, seeds and output positions keep the reference's order (computed up front below)
  std::vector<size_t> order(chunks.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) {
    return chunks[x].a1 - chunks[x].a0 > chunks[y].a1 - chunks[y].a0;
  });
  // HuBERT's feature encoder (and the layers before the gate) on the aux stream beside the U-Net. Measured and removed:
  // issuing it from a later U-Net level on (neutral) and on a CU-masked stream of 64 / 128 CUs (+3.6 ms)
  // Its contractions (issued with ~1.5 ms of slack before the BiGRU) take 64 KB more LDS per workgroup there
  // (HubertRun::lds_pad): one or two of them per CU at most, so the U-Net's latency-bound chain finds free workgroup
  // slots instead of waiting out ~50 us feature-conv workgroups. Same-box A/B (ms/step): r05ac none 13.53 / 13.47,
  // 64 KB 13.28 / 13.35, 88 KB 13.25 / 13.27, 40 KB 13.39 / 13.51; r05ae none 13.53 / 13.54 / 13.48 / 13.51, 64 KB
  // 13.39 / 13.16 / 13.37 / 13.33, 88 KB 13.48 / 13.29. Throttling HuBERT's transformer beside the BiGRU too (r05aa)
  // costs +0.3-0.5 ms: it runs with little slack, so the gated remainder below goes out without the pad.
  // RVCX_AUX_LDS=KB overrides (0: off)
  static const int aux_lds = [] {
    const char* e = rvcx_knob("RVCX_AUX_LDS");
    return (e ? std::max(0, std::atoi(e)) : 64) * 1024;
  }();
  const int front_pad = ax != s ? aux_lds : 0;
  for (size_t i : order) {
    const int64_t len = chunks[i].a1 - chunks[i].a0;
    const int64_t cap_rows = len / 320 + 8;
    cfeats[i] = c.buf<float>("pl.hb" + std::to_string(i), (size_t)cap_rows * E, ax);
    hruns[i] = hubert_front(c, pad32 + chunks[i].a0, len, len, 1, hubert_version_for(c), cfeats[i], cap_rows, ax,
                            front_pad);
    if (chunks.size() == 1) {
      hubert_layers(c, hruns[i], 0, split, ax);
    } else {  // several chunks share the HuBERT workspace: each runs to completion before the next
      hubert_layers(c, hruns[i], 0, HUBERT_LAYERS, ax);
      cL[i] = hubert_tail(c, hruns[i], ax);
    }
  }
  // The rest of HuBERT (one chunk: the layers from the gate on and the tail), issued once: by RMVPE beside its first
  // BiGRU launch, which records c.ev_gate on `main` where the rest may start, or by issue_rest below
  bool rest_issued = false;
  auto hubert_rest = [&](hipStream_t main) {
    rest_issued = true;
    if (chunks.size() != 1) return;
    if (split < HUBERT_LAYERS && ax != main) RVCX_HIP(hipStreamWaitEvent(ax, c.ev_gate, 0));
    hruns[0].lds_pad = 0;
    hubert_layers(c, hruns[0], split, HUBERT_LAYERS, ax);
    cL[0] = hubert_tail(c, hruns[0], ax);
  };
  auto issue_rest = [&] {  // where no BiGRU launch took it: gated here on s
    if (rest_issued) return;
    if (ax != s && c.ev_gate) RVCX_HIP(hipEventRecord(c.ev_gate, s));
    hubert_rest(s);
  };
  // 5. f0 over the whole padded input (pipeline.py:462-472) + get_f0 adjustments (:248-291)
  const int64_t F = 1 + m / W;
  int32_t* pitch = nullptr;
  float* pitchf = nullptr;
  if (guided) {
  double* f0 = c.buf<double>("pl.f0", (size_t)F, s);
  if (o.f0_method >= 1) {
    // CREPE / FCPE over the whole padded input: no BiGRU, so HuBERT's remaining layers go out first and overlap the
    // pitch network's convs on the aux stream
    issue_rest();
    f0_row(c, o, pad32, m, f0, F, "pl.f0f", s);
  } else {
    rmvpe_forward(c, pad32, m, rmvpe_threshold(o), f0, F, nullptr, s, hubert_rest);
  }
  issue_rest();  // RMVPE did not reach a BiGRU launch (cannot happen for valid input): issue it now
  pitch = c.buf<int32_t>("pl.pitch", (size_t)F, s);
  pitchf = c.buf<float>("pl.pitchf", (size_t)F, s);
  pitch_from_f0(c, o, f0, 1, &F, F, pitch, pitchf, f0_out, F, s);
  } else {
    issue_rest();
    if (f0_out) RVCX_HIP(hipMemsetAsync(f0_out, 0, sizeof(double) * (size_t)F, s));
  }
  join_aux(c, s, ax);
  // 6. voice conversion per chunk (pipeline.py:486-512), outputs trimmed t_pad_tgt per side
  const int upp = c.scfg.upp();
  const int I = c.scfg.I;
  // per chunk, in the reference's order: frames T = min(len / 160, 2 L) (vc_forward), noise offsets, seed, output
  // position
  const size_t nch = chunks.size();
  std::vector<int64_t> ez_off(nch), es_off(nch), pos(nch);
  std::vector<uint64_t> cseed(nch);
  int64_t written = 0;
  {
    int64_t ez = 0, es = 0;
    uint64_t sd = seed;
    for (size_t i = 0; i < nch; ++i) {
      ez_off[i] = ez;
      es_off[i] = es;
      cseed[i] = sd;
      pos[i] = written;
      if (nch > 1) {
        const int64_t T = std::min<int64_t>((chunks[i].a1 - chunks[i].a0) / W, 2 * cL[i]);
        ez += (int64_t)I * T;
        es += c.scfg.src_noise_total(1, T);  // this chunk's decoder draws (include/rvcx.h layouts)
        const int64_t keep = T * upp - 2 * o.t_pad_tgt;
        if (keep <= 0) throw Error(RVCX_E_SHAPE, "pipeline: chunk too short for the padding");
        written += keep;
      }
      sd += 0x9E3779B97F4A7C15ull;
    }
    if (written > cap)
      throw Error(RVCX_E_CAPACITY, "pipeline: output needs more than " + std::to_string(cap) + " samples");
  }
  const bool fuse_trim = nch == 1 && o.volume_envelope == 1.0;
  const float* trimmed = out;
  for (size_t i : order) {
    const Chunk& ch = chunks[i];
    const int64_t len = ch.a1 - ch.a0;
    const int64_t cap_vc = (len / W) * upp;
    float* vc = c.buf<float>("pl.vc", (size_t)std::max<int64_t>(cap_vc, 1), s);
    // pitch[:, f_lo:f_hi], then [:p_len] inside voice_conversion with p_len = min(len/160, 2L)
    const int64_t nvc = vc_forward(c, pad32 + ch.a0, len, pitch ? pitch + ch.f_lo : nullptr,
                                   pitchf ? pitchf + ch.f_lo : nullptr, ch.f_hi - ch.f_lo, o.sid,
                                   o.protect, o.index_rate, eps_z ? eps_z + ez_off[i] : nullptr,
                                   eps_src ? eps_src + es_off[i] : nullptr, cseed[i], vc, cap_vc, s, cfeats[i], cL[i],
                                   c.dec_window && !sizing ? o.t_pad_tgt : 0);
    const int64_t keep = nvc - 2 * o.t_pad_tgt;
    if (keep <= 0) throw Error(RVCX_E_SHAPE, "pipeline: chunk too short for the padding");
    if (nch == 1) {
      if (keep > cap)
        throw Error(RVCX_E_CAPACITY, "pipeline: output needs more than " + std::to_string(cap) + " samples");
      written = keep;
    }
    if (fuse_trim)
      trimmed = vc + o.t_pad_tgt;  // one chunk, no envelope: the peak normalisation reads it in place
    else
      RVCX_HIP(hipMemcpyAsync(out + pos[i], vc + o.t_pad_tgt, (size_t)keep * sizeof(float), hipMemcpyDeviceToDevice,
                              s));
  }
  // 7. volume envelope (pipeline.py:545-549) and peak normalisation (:550-552)
  if (o.volume_envelope != 1.0) {
    const int n1 = rms_frame_count(n, 16000), n2 = rms_frame_count(written, c.scfg.sr);
    float* rws = c.buf<float>("pl.rms", (size_t)(n1 + n2), s);
    check(change_rms(filtered, n, (int)n, n, 16000, out, written, (int)written, written, c.scfg.sr,
                     (float)o.volume_envelope, nullptr, rws, s),
          "change_rms");
  }
  float* mx = c.buf<float>("pl.max", peak_normalize_ws_floats(1), s);
  check(peak_normalize(trimmed, written, out, written, (int)written, written, mx, s), "peak_normalize");
  return written;
}

// Batched offline conversion (config C4) of B utterances of nv[b] samples (each one chunk: nv[b] + 160 <= t_max,
// pipeline.py:486-512 with opt_ts empty): one batched HuBERT over the rows (hubert_forward_v), one Synthesizer.infer
// with per-row lengths, and the per-row stages around them (upsample + protect, pitch packing, trim, volume envelope,
// peak normalisation) as one launch set each, driven by device arrays of the rows' lengths. Per utterance the result is
// Pipeline.pipeline's, n_out[b] samples; the batch only widens every GEMM. audio row b at audio + b*lda (fp64), out
// row b at out + b*ldo, f0_out row b at f0_out + b*ldf.
//   - rows of one length throughout (`plain` below) take the equal-length routes: HuBERT without masks, the synthesizer
//     with full lengths, one batched RMVPE straight from the padded input (hidden_out, its salience, only then).
//   - f0: under f0_method 0 rows run through RMVPE's single-row forward, rows of equal length inside the batch together
//     through the batched one, so a row's f0 is the single run's bit for bit; f0_method 4 runs all rows in one ragged
//     pass (rmvpe_forward_v: a length per row in the mel's and the frames' reflect pads, the U-Net's zero padding and
//     the BiGRU), equal to it up to summation order. FCPE likewise: per row under f0_method 3 (bit for bit the single
//     run's), all rows in one ragged pass under f0_method 5 (fcpe_forward_v), equal rows through fcpe_forward_b.
//   - the generator runs over the common window [t_pad_tgt, Tv_max upp - t_pad_tgt) on z * mask, as the reference's
//     own batched Synthesizer.infer does: a shorter row's last frames, within the generator's receptive field of its
//     end, see the zeroed pad frames' activations where a run of that row alone sees the conv's zero padding. The trim
//     removes them only if t_pad_tgt covers the receptive field, so differing lengths with a smaller t_pad_tgt are refused.
void pipeline_forward_rows(Ctx& c, const double* audio, const int64_t* nv, int64_t lda, int B,
                           const rvcx_pipeline_opts& opts, const int32_t* sids, const float* eps_z, const float* eps_src,
                           uint64_t seed, float* out, int64_t ldo, int64_t* n_out, double* f0_out, int64_t ldf,
                           float* hidden_out, hipStream_t s, bool sizing, const int32_t* voices) {
  const Rows rows("pipeline_batch", nv, B, lda, 1);
  const int64_t n_max = rows.n_max;
  const bool equal = rows.equal;
  // The rows of one voice are a contiguous range. Steps 1-2 (high-pass, HuBERT, the pitch network) do not depend on
  // the voice and run once; retrieval, upsample + protect and Synthesizer.infer (steps 3-4) run per voice on its range
  // at the batch's strides; step 5 once. The voices are selected in turn (host only) and the current one comes back.
  struct Group {
    int voice, r0, n;
  };
  std::vector<Group> groups;
  for (int b = 0; b < B; ++b) {
    const int v = voices ? voices[b] : c.cur_voice;
    if (!groups.empty() && groups.back().voice == v) {
      ++groups.back().n;
      continue;
    }
    for (const Group& g : groups)
      if (g.voice == v) throw Error(RVCX_E_INVALID, "pipeline_batch: the rows of one voice must be contiguous");
    if (!c.has_voice(v))
      throw Error(RVCX_E_INVALID, "pipeline_batch: voice " + std::to_string(v) + " does not exist (or was freed)");
    groups.push_back({v, b, 1});
  }
  VoiceScope restore(c);
  int margin = 0;  // the widest receptive field among the voices' generators
  for (auto g = groups.rbegin(); g != groups.rend(); ++g) {  // last to first: the first group's voice stays selected
    c.select_voice(g->voice);
    if (!c.ready[RVCX_MODEL_SYNTH])
      throw Error(RVCX_E_STATE, "pipeline_batch: voice " + std::to_string(g->voice) + " is not finalized");
    for (int b = g->r0; b < g->r0 + g->n; ++b) {
      check_pipeline_opts(c, opts, nv[b]);
      if (opts.t_max > 0 && nv[b] + 160 > opts.t_max)
        throw Error(RVCX_E_INVALID, "pipeline_batch: utterances longer than t_max take the single-utterance path");
      if (sids[b] < 0 || sids[b] >= c.scfg.n_spk) throw Error(RVCX_E_INVALID, "pipeline_batch: sid out of range");
    }
    if (opts.index_rate > 0 && c.ivf->view.d != c.scfg.emb_dim)
      throw Error(RVCX_E_SHAPE, "pipeline: feature index dimension mismatch");
    margin = std::max(margin, dec_margin_frames(c.scfg));
  }
  const VoiceGeom geom = voice_geom(c.scfg);
  for (const Group& g : groups)
    if (g.voice != c.cur_voice && !(voice_geom(c.voices.at(g.voice).scfg) == geom))
      throw Error(RVCX_E_SHAPE, "pipeline_batch: the voices of one batch must agree on sr, upsample product, "
                                "text_enc_hidden_dim, inter_channels, no_f0 and vocoder");
  if (groups.size() > 1 && eps_src && geom.vocoder != 0)
    throw Error(RVCX_E_INVALID, "pipeline_batch: injected source noise with several voices needs the HiFi-GAN-NSF "
                                "noise layout");
  // f0_method 4: all rows in one ragged RMVPE pass; equal lengths (outside the arena query, which sizes the ragged
  // pass) and one row are method 0
  rvcx_pipeline_opts o = opts;
  const bool ragged_f0 = o.f0_method == 4 && B > 1 && (!equal || sizing);
  if (o.f0_method == 4) o.f0_method = 0;
  // f0_method 5: the same for FCPE, one row and (outside the arena query) no other case being method 3
  const bool batch_fcpe = o.f0_method == 5 && B > 1;
  if (o.f0_method == 5) o.f0_method = 3;
  const int E = c.scfg.emb_dim, upp = c.scfg.upp();
  if (!equal && o.t_pad_tgt < (int64_t)margin * upp)
    throw Error(RVCX_E_INVALID, "pipeline_batch: rows of different lengths need t_pad_tgt >= " +
                                    std::to_string((int64_t)margin * upp) +
                                    " samples (the generator's receptive field): a shorter row's last frames differ from "
                                    "a run of that row alone, and only the trim removes them");
  const bool guided = c.scfg.f0;  // no f0, pitch or protect without pitch guidance (pipeline.py:324-365)
  if (hidden_out && !(equal && guided && o.f0_method == 0))
    throw Error(RVCX_E_INVALID, "pipeline_batch: the salience needs equal lengths, RMVPE and a pitch-guided model");
  // rvcx_workspace_bytes sizes the ragged form: masks, the gathered RMVPE group and one single-row RMVPE forward
  const bool plain = equal && !sizing;
  const int64_t W = 160;
  const int64_t m_max = n_max + 2 * o.t_pad;
  const int64_t ldm = (m_max + 7) & ~int64_t(7);
  std::vector<int64_t> mv(B), Fv(B), Lv(B), Tvv(B), keep(B);
  int64_t Tv_max = 0, keep_max = 0;
  for (int b = 0; b < B; ++b) {
    mv[b] = nv[b] + 2 * o.t_pad;
    Fv[b] = 1 + mv[b] / W;
    Lv[b] = hubert_frames(mv[b]);
    Tvv[b] = std::min<int64_t>(mv[b] / W, 2 * Lv[b]);
    if (Tvv[b] <= 0) throw Error(RVCX_E_SHAPE, "pipeline_batch: input shorter than one frame");
    keep[b] = Tvv[b] * upp - 2 * o.t_pad_tgt;
    if (keep[b] <= 0) throw Error(RVCX_E_SHAPE, "pipeline_batch: utterance too short for the padding");
    Tv_max = std::max(Tv_max, Tvv[b]);
    keep_max = std::max(keep_max, keep[b]);
  }
  if (keep_max > ldo) throw Error(RVCX_E_CAPACITY, "pipeline_batch: output rows need " + std::to_string(keep_max));
  const int64_t F_max = 1 + m_max / W, L_max = hubert_frames(m_max);
  if (f0_out && ldf < F_max) throw Error(RVCX_E_CAPACITY, "pipeline_batch: f0 rows need " + std::to_string(F_max));
  // per-row lengths on device: L | Tv | sid | n | keep
  LenCols meta(5, B);
  for (int b = 0; b < B; ++b) {
    meta.at(0, b) = (int32_t)Lv[b];
    meta.at(1, b) = (int32_t)Tvv[b];
    meta.at(2, b) = sids[b];
    meta.at(3, b) = (int32_t)nv[b];
    meta.at(4, b) = (int32_t)keep[b];
  }
  meta.upload(c, "pb.meta", s);
  const int32_t *dL = meta.col(0), *dTv = meta.col(1), *dsid = meta.col(2), *dn = meta.col(3), *dkeep = meta.col(4);
  // 1. zero-phase high-pass + reflect pad per utterance, each with its own length (pipeline.py:439, :459)
  float* pad32 = c.buf<float>("pb.pad32", (size_t)B * ldm, s);
  double* pad64 = c.buf<double>("pb.pad64", (size_t)B * m_max, s);
  // (rows longest first here and in the per-row f0 below: the work buffers the rows share are then never regrown)
  std::vector<int> order(B);
  for (int b = 0; b < B; ++b) order[b] = b;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return nv[x] > nv[y]; });
  for (int b : order)
    highpass_pad(c, audio + (size_t)b * lda, nv[b], o.t_pad, pad64 + (size_t)b * m_max, pad32 + (size_t)b * ldm, s);
  // 2. batched HuBERT on the aux stream beside the f0 of every row, then get_f0's adjustments (pipeline.py:462-472,
  //    :248-291)
  double* f0 = c.buf<double>("pb.f0", (size_t)B * F_max, s);
  float* feats = c.buf<float>("pb.feats", (size_t)B * L_max * E, s);
  hipStream_t ax = fork_aux(c, s);
  hubert_forward_v(c, pad32, mv.data(), ldm, B, hubert_version_for(c), feats, L_max, nullptr, ax, sizing);
  int32_t* pitch = nullptr;
  float* pitchf = nullptr;
  if (guided) {
    if (batch_fcpe) {  // straight from the padded rows; equal lengths take the equal-length batch inside
      fcpe_forward_v(c, pad32, mv.data(), ldm, B, fcpe_threshold(o), 0, f0, F_max, nullptr, 0, s, sizing);
    } else if (o.f0_method >= 1) {  // CREPE / FCPE per utterance (CREPE's frames of all rows would not batch any better)
      for (int b : order)
        f0_row(c, o, pad32 + (size_t)b * ldm, mv[b], f0 + (size_t)b * F_max, Fv[b], "pb.f0f", s);
    } else if (ragged_f0) {
      rmvpe_forward_v(c, pad32, mv.data(), ldm, B, rmvpe_threshold(o), f0, F_max, nullptr, nullptr, 0, s, sizing);
    } else {
      const float thr = rmvpe_threshold(o);
      // rows of equal length together; the groups largest first (rows x frames), so the work buffers a group shares
      // with the next are not regrown
      std::vector<std::vector<int>> groups;
      for (int b = 0; b < B; ++b) {
        bool placed = false;
        for (auto& g : groups)
          if (mv[g[0]] == mv[b]) g.push_back(b), placed = true;
        if (!placed) groups.push_back({b});
      }
      if (sizing) groups.push_back({0});
      std::stable_sort(groups.begin(), groups.end(), [&](const std::vector<int>& x, const std::vector<int>& y) {
        return (int64_t)x.size() * Fv[x[0]] > (int64_t)y.size() * Fv[y[0]];
      });
      for (const auto& g : groups) {
        const int b0 = g[0], ng = (int)g.size();
        if (ng == 1 || (ng == B && plain)) {  // one row, or all of them: in place
          rmvpe_forward_b(c, pad32 + (size_t)b0 * ldm, mv[b0], ldm, ng, thr, f0 + (size_t)b0 * F_max, Fv[b0],
                          ng == B ? hidden_out : nullptr, s);
          continue;
        }
        float* ga = c.buf<float>("pv.grp", (size_t)ng * ldm, s);
        double* gf = c.buf<double>("pv.grpf0", (size_t)ng * F_max, s);
        for (int k = 0; k < ng; ++k)
          RVCX_HIP(hipMemcpyAsync(ga + (size_t)k * ldm, pad32 + (size_t)g[k] * ldm, sizeof(float) * (size_t)mv[b0],
                                  hipMemcpyDeviceToDevice, s));
        rmvpe_forward_b(c, ga, mv[b0], ldm, ng, thr, gf, Fv[b0], nullptr, s);
        for (int k = 0; k < ng; ++k)
          RVCX_HIP(hipMemcpyAsync(f0 + (size_t)g[k] * F_max, gf + (size_t)k * Fv[b0], sizeof(double) * (size_t)Fv[b0],
                                  hipMemcpyDeviceToDevice, s));
      }
    }
    pitch = c.buf<int32_t>("pb.pitch", (size_t)B * F_max, s);
    pitchf = c.buf<float>("pb.pitchf", (size_t)B * F_max, s);
    pitch_from_f0(c, o, f0, B, Fv.data(), F_max, pitch, pitchf, f0_out, ldf, s);
  } else if (f0_out) {
    for (int b = 0; b < B; ++b) RVCX_HIP(hipMemsetAsync(f0_out + (size_t)b * ldf, 0, sizeof(double) * (size_t)Fv[b], s));
  }
  // 3. retrieval over all B*L_max rows (row-wise: a pad row's result is never read), upsample + protect, pitch packing
  //    (pipeline.py:327-362)
  join_aux(c, s, ax);
  const float* fx = feats;
  if (o.index_rate > 0) {
    float* fr = c.buf<float>("pb.feats_idx", (size_t)B * L_max * E, s);
    for (const Group& g : groups) {  // each voice's rows against its own index
      c.select_voice(g.voice);
      const size_t at = (size_t)g.r0 * L_max * E;
      index_retrieve(c, feats + at, (int64_t)g.n * L_max, E, o.index_rate, fr + at, s);
    }
    fx = fr;
  }
  float* phone = c.buf<float>("pb.phone", (size_t)B * Tv_max * E, s);
  int32_t* pc = nullptr;
  float* pf = nullptr;
  if (guided) {
    pc = c.buf<int32_t>("pb.pc", (size_t)B * Tv_max, s);
    pf = c.buf<float>("pb.pf", (size_t)B * Tv_max, s);
    check(pack_pitch(pitch, pitchf, F_max, dTv, (int)Tv_max, pc, pf, B, s), "pack_pitch");
  }
  check(upsample2_protect(fx, feats, dL, (int)L_max, E, phone, dTv, (int)Tv_max,
                          (guided && o.protect < 0.5f) ? pitchf : nullptr, F_max, o.protect, s, B),
        "upsample");
  // 4. one Synthesizer.infer per voice with per-row lengths (pipeline.py:365-372), on its rows at the batch's strides;
  //    the generator over the common window: the samples the trim below keeps. Injected noise is one row per batch row
  //    (the NSF layout, checked above for several voices); drawn noise is keyed by the row within the call, so the
  //    voices after the first draw under seeds of their own.
  const int64_t nvc = Tv_max * upp;
  float* vc = c.buf<float>("pb.vc", (size_t)B * nvc, s);
  // the largest group first: the work buffers the groups share are then never regrown (an arena holds them once)
  std::vector<const Group*> by_size;
  for (const Group& g : groups) by_size.push_back(&g);
  std::stable_sort(by_size.begin(), by_size.end(), [](const Group* x, const Group* y) { return x->n > y->n; });
  for (const Group* gp : by_size) {
    const Group& g = *gp;
    c.select_voice(g.voice);
    const size_t r0 = (size_t)g.r0;
    SynthCall syn;
    syn.B = g.n, syn.T = (int)Tv_max;
    syn.phone = phone + r0 * Tv_max * E, syn.lengths = dTv + r0, syn.sid = dsid + r0;
    if (pc) syn.pitch = pc + r0 * Tv_max, syn.pitchf = pf + r0 * Tv_max;
    syn.eps_z = eps_z ? eps_z + r0 * geom.I * Tv_max : nullptr;
    syn.eps_src = eps_src ? eps_src + r0 * nvc : nullptr;
    syn.seed = seed + 0x9E3779B97F4A7C15ull * (uint64_t)g.r0;
    syn.out = vc + r0 * nvc;
    syn.full_lengths = plain;
    if (o.t_pad_tgt > 0 && c.dec_window && !sizing) syn.win = {o.t_pad_tgt, nvc - o.t_pad_tgt};
    synth_forward(c, syn, s);
  }
  // 5. trim, volume envelope, peak normalisation of every row in one launch set each (pipeline.py:545-552)
  float* mx = c.buf<float>("pb.max", peak_normalize_ws_floats(B), s);
  if (o.volume_envelope == 1.0) {  // trim + normalise in one pass over all rows
    check(peak_normalize(vc + o.t_pad_tgt, nvc, out, ldo, dkeep, keep_max, mx, s, B), "peak_normalize");
  } else {
    RVCX_HIP(hipMemcpy2DAsync(out, ldo * sizeof(float), vc + o.t_pad_tgt, nvc * sizeof(float), keep_max * sizeof(float),
                              B, hipMemcpyDeviceToDevice, s));
    const int nrms = rms_frame_count(n_max, 16000) + rms_frame_count(keep_max, c.scfg.sr);
    float* rws = c.buf<float>("pb.rms", (size_t)B * nrms, s);
    check(change_rms(pad64 + o.t_pad, m_max, dn, n_max, 16000, out, ldo, dkeep, keep_max, c.scfg.sr,
                     (float)o.volume_envelope, nullptr, rws, s, B),
          "change_rms");
    check(peak_normalize(out, ldo, out, ldo, dkeep, keep_max, mx, s, B), "peak_normalize");
  }
  for (int b = 0; b < B; ++b) n_out[b] = keep[b];
}

// B equal-length utterances of n samples: the rows above with one length; returns the rows' output length
int64_t pipeline_forward_batch(Ctx& c, const double* audio, int64_t n, int64_t lda, int B, const rvcx_pipeline_opts& o,
                               const int32_t* sids, const float* eps_z, const float* eps_src, uint64_t seed,
                               float* out, int64_t ldo, double* f0_out, float* hidden_out, hipStream_t s) {
  if (B < 1) throw Error(RVCX_E_INVALID, "pipeline_batch: B < 1");
  const std::vector<int64_t> nv((size_t)B, n);
  std::vector<int64_t> n_out((size_t)B);
  pipeline_forward_rows(c, audio, nv.data(), lda, B, o, sids, eps_z, eps_src, seed, out, ldo, n_out.data(), f0_out,
                        1 + (n + 2 * o.t_pad) / 160, hidden_out, s, false);
  return n_out[0];
}

namespace {
// rvcx_workspace_bytes plans from an empty, internally allocated pool: the caller's arena is detached for the scope and
// attached again after (its regions are carved anew by the next call), and the pool the plan took is dropped
struct SizingScope {
  Ctx& c;
  char* const arena;
  const size_t arena_bytes;
  explicit SizingScope(Ctx& cc) : c(cc), arena(cc.arena), arena_bytes(cc.arena_bytes) {
    c.release_pool();
    c.arena = nullptr;
    c.arena_bytes = 0;
  }
  ~SizingScope() {
    (void)hipDeviceSynchronize();  // release_pool without its throw: every measurement has synchronised its stream
    c.drop_pool();
    c.arena = arena;
    c.arena_bytes = arena_bytes;
  }
};
}  // namespace

int64_t pipeline_workspace_bytes(Ctx& c, int B, int64_t n, const rvcx_pipeline_opts& opts, hipStream_t s) {
  // the call itself on zero audio, in its sizing form; the buffers outlive the scope, which synchronises the device
  // before they are freed
  DevBuf audio, out;
  SizingScope scope(c);
  const int64_t m = n + 2 * opts.t_pad;
  const int64_t cap = (m / 160 + (opts.t_center > 0 ? n / opts.t_center : 0) + 2) * c.scfg.upp();
  RVCX_HIP(hipMalloc(&audio.p, sizeof(double) * (size_t)(B * n)));
  RVCX_HIP(hipMalloc(&out.p, sizeof(float) * (size_t)(B * cap)));
  RVCX_HIP(hipMemsetAsync(audio.p, 0, sizeof(double) * (size_t)(B * n), s));
  auto measure = [&](const rvcx_pipeline_opts& o) {
    if (B == 1) {
      pipeline_forward_ex(c, static_cast<const double*>(audio.p), n, o, nullptr, nullptr, 0, static_cast<float*>(out.p),
                          cap, nullptr, s, true);
    } else {
      // B rows of n samples in the batched pipeline's sizing form: run as a ragged batch (masks,
      // the gathered RMVPE group and one single-row RMVPE forward), whose regions hold the equal-length routes too
      std::vector<int32_t> sids((size_t)B, o.sid);
      std::vector<int64_t> nv((size_t)B, n), no((size_t)B);
      pipeline_forward_rows(c, static_cast<const double*>(audio.p), nv.data(), n, B, o, sids.data(), nullptr, nullptr, 0,
                            static_cast<float*>(out.p), cap, no.data(), nullptr, 0, nullptr, s, true);
    }
    RVCX_HIP(hipStreamSynchronize(s));
    int64_t carved = (int64_t)c.carved;
    if (B > 1) {
      // a ragged batch walks its rows' front ends in another order than the call above, and the split-K slab all
      // convs share is regrown whenever a later conv needs a larger one: room for one regrowth per row and stream
      for (const char* slab : {"conv.splitk", "conv.splitk.aux"})
        if (c.ws.count(slab) && c.ws[slab]) carved += (int64_t)B * (int64_t)c.ws[slab]->bytes;
    }
    return carved;
  };
  int64_t need = measure(opts);
  if (opts.f0_method == 3 || opts.f0_method == 5) {
    // FCPE's scratch is carved in place of RMVPE's, which can be the larger: the size also holds the same call
    // with the default f0 method, so an arena sized for "fcpe" serves a caller that switches back
    rvcx_pipeline_opts o0 = opts;
    o0.f0_method = 0;
    c.release_pool();
    need = std::max(need, measure(o0));
  }
  // the per-chunk HuBERT feature buffers (pl.hb<i>) sum to the same total over any split plan up to one row and
  // the 256-B rounding per chunk
  if (B == 1 && opts.t_max > 0 && n + 160 > opts.t_max && opts.t_center > 0) {
    const int64_t nts = n > opts.t_center ? (n - 1 - opts.t_center) / opts.t_center + 1 : 0;
    need += (nts + 1) * ((int64_t)c.scfg.emb_dim * 4 + 512);
  }
  return need;
}

rvcx_pipeline_opts default_pipeline_opts() {
  rvcx_pipeline_opts o;
  std::memset(&o, 0, sizeof(o));
  o.version = 0;
  o.protect = 0.33f;
  o.rmvpe_threshold = RMVPE_THRESHOLD;
  o.t_pad = 16000;
  o.t_pad_tgt = 48000;
  o.t_query = 16000 * 6;
  o.t_center = 16000 * 38;
  o.t_max = 16000 * 41;
  o.f0_autotune_strength = 1.0;
  o.proposed_pitch_threshold = 155.0;
  o.volume_envelope = 1.0;
  o.fcpe_threshold = FCPE_THRESHOLD;
  return o;
}

}  // namespace rvcx
