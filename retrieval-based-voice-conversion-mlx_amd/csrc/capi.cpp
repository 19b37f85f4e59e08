// extern "C" boundary of the product ABI (include/rvcx.h); the kernel-level test entries (include/rvcx_test.h) are
// capi_test.cpp. Every entry point converts C++ exceptions into an rvcx_status and stores the message for
// rvcx_last_error (guard, capi_common.h).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

#include "capi_common.h"
#include "rows.h"

extern char** environ;

using namespace rvcx;

namespace rvcx {
// read at every knob read (not cached): most knobs are read once into a static at their first use, the BiGRU's
// fault-injection hook (RVCX_GRU_SPIN_LIMIT) per call, so a test can set and clear it with the opt-in
static bool experimental_on() {
  const char* e = std::getenv("RVCX_EXPERIMENTAL");
  return e && std::atoi(e) == 1;
}
const char* rvcx_knob(const char* name) { return experimental_on() ? std::getenv(name) : nullptr; }
}  // namespace rvcx

namespace {
// the three models every pipeline entry runs
bool pipeline_ready(const rvcx_ctx* c) {
  return c->ready[RVCX_MODEL_SYNTH] && c->ready[RVCX_MODEL_HUBERT] && c->ready[RVCX_MODEL_RMVPE];
}
}  // namespace

extern "C" {

int rvcx_create(rvcx_ctx** out, int device) {
  if (!out) return RVCX_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return RVCX_E_HIP;
  auto* c = new rvcx_ctx();
  c->device = device;
  if (const char* e = rvcx_knob("RVCX_DEC_WINDOW")) c->dec_window = std::atoi(e) != 0;  // A/B aid (rvcx_set_dec_window)
  *out = c;
  return RVCX_OK;
}

int rvcx_destroy(rvcx_ctx* ctx) {
  if (!ctx) return RVCX_E_INVALID;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  delete ctx;
  return RVCX_OK;
}

const char* rvcx_last_error(const rvcx_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int rvcx_set_synth_config(rvcx_ctx* ctx, const rvcx_synth_desc* d) {
  return guard(ctx, [&] {
    ctx->scfg = synth_cfg_of(d);
    ctx->synth_cfg_set = true;
    ctx->ready[RVCX_MODEL_SYNTH] = false;
  });
}

int rvcx_upload(rvcx_ctx* ctx, int model, const char* name, const float* host, const int64_t* shape, int ndim) {
  return guard(ctx, [&] {
    if (model < 0 || model > RVCX_MODEL_FCPE || !name || !host || (ndim > 0 && !shape) || ndim < 0 || ndim > 8)
      throw Error(RVCX_E_INVALID, "rvcx_upload: bad arguments");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
      if (shape[i] < 0) throw Error(RVCX_E_INVALID, "negative dim");
      t.shape.push_back(shape[i]);
      n *= (size_t)shape[i];
    }
    t.v.assign(host, host + n);
    ctx->host[model][name] = std::move(t);
    ctx->ready[model] = false;
  });
}

int rvcx_finalize(rvcx_ctx* ctx, int model) {
  return guard(ctx, [&] {
    set_device(ctx);
    if (model == RVCX_MODEL_SYNTH) {  // packed into the current voice's own tensor map
      struct Packing {
        bool& f;
        explicit Packing(bool& b) : f(b) { f = true; }
        ~Packing() { f = false; }
      } packing(ctx->packing_synth);
      finalize_synth(*ctx);
    } else if (model == RVCX_MODEL_HUBERT) {
      finalize_hubert(*ctx);
    } else if (model == RVCX_MODEL_RMVPE) {
      finalize_rmvpe(*ctx);
    } else if (model == RVCX_MODEL_CREPE) {
      finalize_crepe(*ctx);
    } else if (model == RVCX_MODEL_FCPE) {
      finalize_fcpe(*ctx);
    } else {
      throw Error(RVCX_E_INVALID, "unknown model");
    }
    RVCX_HIP(hipDeviceSynchronize());
    ctx->ready[model] = true;
  });
}

int rvcx_synth_upp(const rvcx_ctx* ctx) { return ctx ? ctx->scfg.upp() : 0; }

// ------------------------------------------------------------------ voice bank
int rvcx_voice_new(rvcx_ctx* ctx, int* voice) {
  return guard(ctx, [&] {
    if (!voice) throw Error(RVCX_E_INVALID, "rvcx_voice_new: null output");
    *voice = ctx->new_voice();
  });
}

int rvcx_voice_select(rvcx_ctx* ctx, int voice) {
  return guard(ctx, [&] { ctx->select_voice(voice); });
}

int rvcx_voice_current(const rvcx_ctx* ctx, int* voice) {
  if (!ctx || !voice) return RVCX_E_INVALID;
  *voice = ctx->cur_voice;
  return RVCX_OK;
}

int rvcx_voice_info(rvcx_ctx* ctx, int voice, rvcx_voice_desc* desc) {
  return guard(ctx, [&] {
    if (!desc) throw Error(RVCX_E_INVALID, "rvcx_voice_info: null desc");
    if (!ctx->has_voice(voice)) throw Error(RVCX_E_INVALID, "rvcx_voice_info: the voice does not exist (or was freed)");
    std::memset(desc, 0, sizeof(*desc));
    const bool cur = voice == ctx->cur_voice;
    const Voice* v = cur ? nullptr : &ctx->voices.at(voice);
    const SynthCfg& g = cur ? ctx->scfg : v->scfg;
    desc->config_set = (cur ? ctx->synth_cfg_set : v->synth_cfg_set) ? 1 : 0;
    desc->ready = (cur ? ctx->ready[RVCX_MODEL_SYNTH] : v->ready) ? 1 : 0;
    if (desc->config_set) {
      rvcx_synth_desc& d = desc->synth;
      d.inter_channels = g.I, d.hidden_channels = g.H, d.filter_channels = g.F;
      d.n_heads = g.n_heads, d.n_layers = g.n_layers, d.kernel_size = g.ksize;
      d.n_resblocks = (int)g.rb_k.size();
      d.n_dilations = g.rb_d.empty() ? 0 : (int)g.rb_d[0].size();
      for (size_t j = 0; j < g.rb_k.size(); ++j) {
        d.resblock_kernel_sizes[j] = g.rb_k[j];
        for (size_t m = 0; m < g.rb_d[j].size(); ++m) d.resblock_dilation_sizes[j][m] = g.rb_d[j][m];
      }
      d.n_upsample = (int)g.ups.size();
      for (size_t i = 0; i < g.ups.size(); ++i) d.upsample_rates[i] = g.ups[i], d.upsample_kernel_sizes[i] = g.up_k[i];
      d.upsample_initial_channel = g.C0;
      d.spk_embed_dim = g.n_spk, d.gin_channels = g.gin, d.sr = g.sr, d.text_enc_hidden_dim = g.emb_dim;
      d.no_f0 = g.f0 ? 0 : 1, d.vocoder = g.vocoder;
    }
    if (const IvfIndex* ix = cur ? ctx->ivf.get() : v->ivf.get()) {
      desc->index_d = ix->view.d, desc->index_ntotal = ix->view.ntotal;
      desc->index_nlist = ix->view.nlist, desc->index_nprobe = ix->view.nprobe;
    }
    ctx->voice_bytes(voice, &desc->weight_bytes, &desc->split_bytes);
  });
}

int rvcx_voice_free(rvcx_ctx* ctx, int voice) {
  return guard(ctx, [&] {
    RVCX_HIP(hipSetDevice(ctx->device));
    ctx->free_voice(voice);
  });
}

int rvcx_rt_set_voice(rvcx_ctx* ctx, rvcx_rt* rt, int stream_index, int voice) {
  return guard(ctx, [&] {
    if (!rt || !rt->s) throw Error(RVCX_E_INVALID, "rt_set_voice: null stream group");
    rt_set_voice(*ctx, *rt->s, stream_index, voice);
  });
}

int rvcx_rt_get_voices(const rvcx_rt* rt, int32_t* out) {
  if (!rt || !rt->s || !out) return RVCX_E_INVALID;
  rt_get_voices(*rt->s, out);
  return RVCX_OK;
}

int rvcx_hubert(rvcx_ctx* ctx, const float* d_audio, int64_t n, int version, float* d_feats, int64_t cap_rows,
                int64_t* rows_out, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_HUBERT]) throw Error(RVCX_E_STATE, "hubert weights not finalized");
    if (!d_audio || !d_feats || n <= 0) throw Error(RVCX_E_INVALID, "rvcx_hubert: bad arguments");
    set_device(ctx);
    const int64_t L = hubert_forward(*ctx, d_audio, n, version == 1 ? 1 : 2, d_feats, cap_rows,
                                     static_cast<hipStream_t>(stream));
    if (rows_out) *rows_out = L;
  });
}

int rvcx_rmvpe(rvcx_ctx* ctx, const float* d_audio, int64_t n, float thred, double* d_f0, int64_t cap_frames,
               int64_t* frames_out, float* d_hidden, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_RMVPE]) throw Error(RVCX_E_STATE, "rmvpe weights not finalized");
    if (!d_audio || !d_f0 || n <= 0) throw Error(RVCX_E_INVALID, "rvcx_rmvpe: bad arguments");
    set_device(ctx);
    const int64_t F = rmvpe_forward(*ctx, d_audio, n, thred, d_f0, cap_frames, d_hidden,
                                    static_cast<hipStream_t>(stream));
    if (frames_out) *frames_out = F;
  });
}

int rvcx_crepe(rvcx_ctx* ctx, const float* d_audio, int64_t n, float f0_min, float f0_max, float threshold,
               float* d_f0, float* d_periodicity, float* d_probs, int64_t cap_frames, int64_t* frames_out,
               void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_CREPE]) throw Error(RVCX_E_STATE, "crepe weights not finalized");
    if (!d_audio || !d_f0 || n <= 0) throw Error(RVCX_E_INVALID, "rvcx_crepe: bad arguments");
    if (cap_frames < 1 + n / 160) throw Error(RVCX_E_SHAPE, "rvcx_crepe: output capacity below 1 + n/160 frames");
    set_device(ctx);
    const int64_t F = crepe_forward(*ctx, d_audio, n, f0_min, f0_max, threshold, d_f0, nullptr, d_periodicity,
                                    d_probs, static_cast<hipStream_t>(stream));
    if (frames_out) *frames_out = F;
  });
}

int rvcx_crepe_ex(rvcx_ctx* ctx, const float* d_audio, int64_t n, float f0_min, float f0_max, float threshold,
                  int semantics, const float* d_dither, float* d_f0, float* d_periodicity, float* d_probs,
                  int64_t cap_frames, int64_t* frames_out, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_CREPE]) throw Error(RVCX_E_STATE, "crepe weights not finalized");
    if (!d_audio || !d_f0 || n <= 0 || semantics < 0 || semantics > 1 || (d_dither && semantics != 1))
      throw Error(RVCX_E_INVALID, "rvcx_crepe_ex: bad arguments");
    if (cap_frames < 1 + n / 160) throw Error(RVCX_E_SHAPE, "rvcx_crepe_ex: output capacity below 1 + n/160 frames");
    set_device(ctx);
    const int64_t F = crepe_forward(*ctx, d_audio, n, f0_min, f0_max, threshold, d_f0, nullptr, d_periodicity, d_probs,
                                    static_cast<hipStream_t>(stream), semantics, d_dither);
    if (frames_out) *frames_out = F;
  });
}

int rvcx_crepe_decode(rvcx_ctx* ctx, const float* d_probs, int64_t F, float f0_min, float f0_max, float threshold,
                      int semantics, const float* d_dither, float* d_f0, float* d_periodicity, void* stream) {
  return guard(ctx, [&] {
    if (!d_probs || !d_f0 || F <= 0 || F > INT32_MAX / 360 || semantics < 0 || semantics > 1 ||
        (d_dither && semantics != 1) || !(f0_min > 0.f) || !(f0_max >= f0_min))
      throw Error(RVCX_E_INVALID, "rvcx_crepe_decode: bad arguments");
    set_device(ctx);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    float* f0r = ctx->buf<float>("cr.f0raw", (size_t)F, s);
    float* pr = ctx->buf<float>("cr.perraw", (size_t)F, s);
    const double off = 1997.3794084376191;
    if (semantics == 1) {
      const int minidx = (int)std::min(360.0, std::max(0.0, std::floor((1200.0 * std::log2(f0_min / 10.0) - off) / 20.0)));
      const int maxidx = (int)std::min(360.0, std::max(0.0, std::ceil((1200.0 * std::log2(f0_max / 10.0) - off) / 20.0)));
      if (minidx >= maxidx) throw Error(RVCX_E_INVALID, "rvcx_crepe_decode: [f0_min, f0_max] covers no pitch bin");
      float* lp = ctx->buf<float>("cr.lp", (size_t)F * 360, s);
      int* ptr = ctx->buf<int>("cr.ptr", (size_t)F * 360, s);
      int* bins = ctx->buf<int>("cr.bins", (size_t)F, s);
      check(crepe_decode_viterbi(d_probs, (int)F, minidx, maxidx, d_dither, threshold, lp, ptr, bins, f0r, pr, d_f0,
                                 nullptr, d_periodicity, s), "crepe_decode_viterbi");
    } else {
      check(crepe_decode(d_probs, (int)F, 1200.0 * std::log2(f0_min / 10.0), 1200.0 * std::log2(f0_max / 10.0),
                         threshold, f0r, pr, d_f0, nullptr, d_periodicity, s), "crepe_decode");
    }
  });
}

int rvcx_set_fcpe_config(rvcx_ctx* ctx, const rvcx_fcpe_desc* d) {
  return guard(ctx, [&] {
    if (!d) throw Error(RVCX_E_INVALID, "null desc");
    FcpeCfg g;
    g.sr = d->sampling_rate;
    g.n_fft = d->n_fft;
    g.win = d->win_size;
    g.hop = d->hop_size;
    g.n_mels = d->num_mels;
    g.fmin = d->fmin;
    g.fmax = d->fmax;
    g.n_layers = d->n_layers;
    g.n_chans = d->n_chans;
    g.out_dims = d->out_dims;
    if (g.sr < 1 || g.n_fft < 1 || g.win < 1 || g.hop < 1 || g.n_mels < 1 || g.n_layers < 1 || g.n_layers > 64 ||
        g.n_chans < 1 || g.out_dims < 1)
      throw Error(RVCX_E_INVALID, "rvcx_set_fcpe_config: sizes must be positive");
    ctx->fcfg = g;
    ctx->ready[RVCX_MODEL_FCPE] = false;
  });
}

int rvcx_fcpe(rvcx_ctx* ctx, const float* d_audio, int64_t n, float threshold, int decoder_mode, int interp_uv,
              int64_t pad_to, double* d_f0, float* d_salience, int64_t cap_frames, int64_t* frames_out, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_FCPE]) throw Error(RVCX_E_STATE, "fcpe weights not finalized");
    if (!d_audio || !d_f0 || n <= 0 || decoder_mode < 0 || decoder_mode > 1 || pad_to < 0)
      throw Error(RVCX_E_INVALID, "rvcx_fcpe: bad arguments");
    set_device(ctx);
    const int64_t F = fcpe_forward(*ctx, d_audio, n, threshold, decoder_mode, interp_uv ? 1 : 0, pad_to, d_f0,
                                   d_salience, cap_frames, static_cast<hipStream_t>(stream));
    if (frames_out) *frames_out = F;
  });
}

int rvcx_fcpe_b(rvcx_ctx* ctx, const float* d_audio, int64_t n, int64_t ld, int B, float threshold, int decoder_mode,
                double* d_f0, float* d_salience, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_FCPE]) throw Error(RVCX_E_STATE, "fcpe weights not finalized");
    if (!d_audio || !d_f0 || n <= 0 || B < 1 || ld < n || decoder_mode < 0 || decoder_mode > 1)
      throw Error(RVCX_E_INVALID, "rvcx_fcpe_b: bad arguments");
    set_device(ctx);
    fcpe_forward_b(*ctx, d_audio, n, ld, B, threshold, decoder_mode, d_f0, fcpe_frames(*ctx, n), d_salience,
                   static_cast<hipStream_t>(stream));
  });
}

int rvcx_fcpe_batch_v(rvcx_ctx* ctx, const float* d_audio, const int64_t* n, int64_t lda, int B, float threshold,
                      int decoder_mode, double* d_f0, int64_t ldf, int64_t* F_out, float* d_salience,
                      int64_t ld_sal_frames, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_FCPE]) throw Error(RVCX_E_STATE, "fcpe weights not finalized");
    if (!d_audio || !d_f0 || !n || B < 1 || ldf < 1 || (d_salience && ld_sal_frames < 1) || decoder_mode < 0 ||
        decoder_mode > 1)
      throw Error(RVCX_E_INVALID, "rvcx_fcpe_batch_v: bad arguments");
    Rows("rvcx_fcpe_batch_v", n, B, lda, 1);
    set_device(ctx);
    fcpe_forward_v(*ctx, d_audio, n, lda, B, threshold, decoder_mode, d_f0, ldf, d_salience, ld_sal_frames,
                   static_cast<hipStream_t>(stream));
    if (F_out)
      for (int b = 0; b < B; ++b) F_out[b] = fcpe_frames(*ctx, n[b]);
  });
}

int rvcx_fcpe_decode(rvcx_ctx* ctx, const float* d_salience, int64_t F, float threshold, int decoder_mode,
                     int interp_uv, int64_t pad_to, double* d_f0, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_FCPE]) throw Error(RVCX_E_STATE, "fcpe weights not finalized");
    if (!d_salience || !d_f0 || F <= 0 || decoder_mode < 0 || decoder_mode > 1 || pad_to < 0)
      throw Error(RVCX_E_INVALID, "rvcx_fcpe_decode: bad arguments");
    set_device(ctx);
    fcpe_decode_run(*ctx, d_salience, F, threshold, decoder_mode, interp_uv ? 1 : 0, pad_to, d_f0,
                    static_cast<hipStream_t>(stream));
  });
}

int rvcx_split_audio(rvcx_ctx* ctx, const double* d_audio, int64_t n, int sr, double silence_thresh_db,
                     int min_silence_len_ms, int64_t* intervals, int64_t cap, int64_t* count, void* stream) {
  return guard(ctx, [&] {
    if (!d_audio || !intervals || n <= 0 || sr <= 0 || cap < 0 || !count)
      throw Error(RVCX_E_INVALID, "rvcx_split_audio: bad arguments");
    set_device(ctx);
    *count = split_intervals(*ctx, d_audio, n, sr, silence_thresh_db, min_silence_len_ms, intervals, cap,
                             static_cast<hipStream_t>(stream));
  });
}

int rvcx_hubert_batch(rvcx_ctx* ctx, const float* d_audio, int64_t n, int64_t lda, int B, int version, float* d_feats,
                      int64_t cap_rows, int64_t* rows_out, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_HUBERT]) throw Error(RVCX_E_STATE, "hubert weights not finalized");
    if (!d_audio || !d_feats || n <= 0 || B < 1 || lda < n) throw Error(RVCX_E_INVALID, "rvcx_hubert_batch: bad arguments");
    set_device(ctx);
    const int64_t L = hubert_forward_b(*ctx, d_audio, n, lda, B, version == 1 ? 1 : 2, d_feats, cap_rows,
                                       static_cast<hipStream_t>(stream));
    if (rows_out) *rows_out = L;
  });
}

int rvcx_hubert_batch_v(rvcx_ctx* ctx, const float* d_audio, const int64_t* n, int64_t lda, int B, int version,
                        float* d_feats, int64_t ld_rows, int64_t* L_out, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_HUBERT]) throw Error(RVCX_E_STATE, "hubert weights not finalized");
    if (!d_audio || !d_feats || !n || B < 1 || ld_rows < 1) throw Error(RVCX_E_INVALID, "rvcx_hubert_batch_v: bad arguments");
    Rows("rvcx_hubert_batch_v", n, B, lda, 1);
    set_device(ctx);
    hubert_forward_v(*ctx, d_audio, n, lda, B, version == 1 ? 1 : 2, d_feats, ld_rows, L_out,
                     static_cast<hipStream_t>(stream));
  });
}

int rvcx_rmvpe_batch(rvcx_ctx* ctx, const float* d_audio, int64_t n, int64_t lda, int B, float thred, double* d_f0,
                     int64_t cap_frames, int64_t* frames_out, float* d_hidden, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_RMVPE]) throw Error(RVCX_E_STATE, "rmvpe weights not finalized");
    if (!d_audio || !d_f0 || n <= 0 || B < 1 || lda < n) throw Error(RVCX_E_INVALID, "rvcx_rmvpe_batch: bad arguments");
    set_device(ctx);
    const int64_t F = rmvpe_forward_b(*ctx, d_audio, n, lda, B, thred, d_f0, cap_frames, d_hidden,
                                      static_cast<hipStream_t>(stream));
    if (frames_out) *frames_out = F;
  });
}

int rvcx_rmvpe_batch_v(rvcx_ctx* ctx, const float* d_audio, const int64_t* n, int64_t lda, int B, float thred,
                       double* d_f0, int64_t ldf, int64_t* F_out, float* d_hidden, int64_t ld_hidden_frames,
                       void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_RMVPE]) throw Error(RVCX_E_STATE, "rmvpe weights not finalized");
    if (!d_audio || !d_f0 || !n || B < 1 || ldf < 1 || (d_hidden && ld_hidden_frames < 1))
      throw Error(RVCX_E_INVALID, "rvcx_rmvpe_batch_v: bad arguments");
    Rows("rvcx_rmvpe_batch_v", n, B, lda, 1);
    set_device(ctx);
    rmvpe_forward_v(*ctx, d_audio, n, lda, B, thred, d_f0, ldf, F_out, d_hidden, ld_hidden_frames,
                    static_cast<hipStream_t>(stream));
  });
}

int rvcx_rmvpe_decode(rvcx_ctx* ctx, const float* d_hidden, int64_t F, float thred, double* d_f0, void* stream) {
  return guard(ctx, [&] {
    if (!d_hidden || !d_f0 || F < 0) throw Error(RVCX_E_INVALID, "rvcx_rmvpe_decode: bad arguments");
    if (F == 0) return;
    set_device(ctx);
    check(rmvpe_decode(d_hidden, (int)F, 360, thred, d_f0, static_cast<hipStream_t>(stream)), "rmvpe_decode");
  });
}

int rvcx_f0_post(rvcx_ctx* ctx, const double* d_f0, int64_t F, double semitones, int32_t* d_coarse, float* d_pitchf,
                 double* d_f0_shifted, void* stream) {
  return guard(ctx, [&] {
    if (!d_f0 || !d_coarse || !d_pitchf || F < 0) throw Error(RVCX_E_INVALID, "rvcx_f0_post: bad arguments");
    set_device(ctx);
    check(f0_post(d_f0, (int)F, std::pow(2.0, semitones / 12.0), d_coarse, d_pitchf, d_f0_shifted,
                  static_cast<hipStream_t>(stream)),
          "f0_post");
  });
}

int rvcx_f0_autotune(rvcx_ctx* ctx, double* d_f0, int64_t F, double strength, int skip_unvoiced, void* stream) {
  return guard(ctx, [&] {
    if (!d_f0 || F < 0) throw Error(RVCX_E_INVALID, "rvcx_f0_autotune: bad arguments");
    if (F == 0) return;
    set_device(ctx);
    check(f0_autotune(d_f0, (int)F, strength, skip_unvoiced, static_cast<hipStream_t>(stream)), "f0_autotune");
  });
}

int rvcx_synth_infer(rvcx_ctx* ctx, int B, int T, const float* d_phone, const int32_t* d_lengths,
                     const int32_t* d_pitch, const float* d_pitchf, const int32_t* d_sid, const float* d_eps_z,
                     const float* d_eps_src, uint64_t seed, float* d_out, float* d_zp, float* d_z, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_SYNTH]) throw Error(RVCX_E_STATE, "synthesizer weights not finalized");
    if (B <= 0 || T <= 0 || !d_phone || !d_lengths || !d_sid || !d_out)
      throw Error(RVCX_E_INVALID, "rvcx_synth_infer: bad arguments");
    if (ctx->scfg.f0 && (!d_pitch || !d_pitchf))
      throw Error(RVCX_E_INVALID, "rvcx_synth_infer: a pitch-guided model needs pitch and pitchf");
    if (!ctx->scfg.f0) d_pitch = nullptr, d_pitchf = nullptr;  // Synthesizer.infer ignores them (:233-239)
    set_device(ctx);
    SynthCall syn;
    syn.B = B, syn.T = T;
    syn.phone = d_phone, syn.lengths = d_lengths, syn.pitch = d_pitch, syn.pitchf = d_pitchf, syn.sid = d_sid;
    syn.eps_z = d_eps_z, syn.eps_src = d_eps_src, syn.seed = seed;
    syn.out = d_out, syn.zp_out = d_zp, syn.z_out = d_z;
    synth_forward(*ctx, syn, static_cast<hipStream_t>(stream));
  });
}

int rvcx_synth_infer_ex(rvcx_ctx* ctx, int B, int T, const float* d_phone, const int32_t* d_lengths,
                        const int32_t* d_pitch, const float* d_pitchf, const int32_t* d_sid, double rate,
                        const float* d_eps_z, const float* d_eps_src, uint64_t seed, float* d_out, float* d_zp,
                        float* d_z, float* d_m_p, float* d_logs_p, int* t_out, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_SYNTH]) throw Error(RVCX_E_STATE, "synthesizer weights not finalized");
    if (B <= 0 || T <= 0 || !d_phone || !d_lengths || !d_sid || !d_out)
      throw Error(RVCX_E_INVALID, "rvcx_synth_infer_ex: bad arguments");
    if (ctx->scfg.f0 && (!d_pitch || !d_pitchf))
      throw Error(RVCX_E_INVALID, "rvcx_synth_infer_ex: a pitch-guided model needs pitch and pitchf");
    if (!ctx->scfg.f0) d_pitch = nullptr, d_pitchf = nullptr;
    // head = int(z_p.shape[2] * (1.0 - rate)) (synthesizers.py:231), then Python's slice [head:]: a negative head
    // (rate > 1) keeps the last -head frames (all T when -head >= T); rate < 0: no rate (None)
    int head = 0;
    if (rate >= 0.0) {
      const double h = (double)T * (1.0 - rate);
      if (std::isnan(h)) throw Error(RVCX_E_INVALID, "rvcx_synth_infer_ex: rate is not a number");
      const double ht = std::trunc(h);  // int(): toward zero
      head = ht >= 0.0 ? (int)std::min(ht, (double)T) : (int)std::max(0.0, (double)T + ht);
      if (head >= T) throw Error(RVCX_E_SHAPE, "rvcx_synth_infer_ex: rate keeps no frame (the reference's slice is empty)");
    }
    set_device(ctx);
    SynthCall syn;
    syn.B = B, syn.T = T;
    syn.phone = d_phone, syn.lengths = d_lengths, syn.pitch = d_pitch, syn.pitchf = d_pitchf, syn.sid = d_sid;
    syn.eps_z = d_eps_z, syn.eps_src = d_eps_src, syn.seed = seed;
    syn.out = d_out, syn.zp_out = d_zp, syn.z_out = d_z, syn.mp_out = d_m_p, syn.logsp_out = d_logs_p;
    syn.head = head;
    synth_forward(*ctx, syn, static_cast<hipStream_t>(stream));
    if (t_out) *t_out = T - head;
  });
}

int rvcx_dec_only(rvcx_ctx* ctx, int B, int T, const float* d_z, const float* d_f0, const int32_t* d_sid,
                  const float* d_eps_src, uint64_t seed, float* d_out, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_SYNTH]) throw Error(RVCX_E_STATE, "synthesizer weights not finalized");
    if (B <= 0 || T <= 0 || !d_z || !d_sid || !d_out || (ctx->scfg.f0 && !d_f0))
      throw Error(RVCX_E_INVALID, "rvcx_dec_only: bad arguments");
    set_device(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int I = ctx->scfg.I;
    float* zt = ctx->buf<float>("dec_only.z", (size_t)B * T * I, s);
    check(transpose_bct_btc(d_z, zt, B, I, T, s), "transpose");
    float* g = ctx->buf<float>("dec_only.g", (size_t)B * ctx->scfg.gin, s);
    check(gather_rows(ctx->W("emb_g"), ctx->scfg.gin, d_sid, g, B, ctx->scfg.gin, s), "emb_g");
    DecCall dec;
    dec.B = B, dec.T = T;
    dec.z_btc = zt, dec.f0 = d_f0, dec.g = g, dec.eps_src = d_eps_src, dec.seed = seed;
    dec.out = d_out;
    dec_forward(*ctx, dec, s);
  });
}

int rvcx_voice_conversion(rvcx_ctx* ctx, const float* d_audio, int64_t n, const int32_t* d_pitch,
                          const float* d_pitchf, int sid, float protect, double index_rate, const float* d_eps_z,
                          const float* d_eps_src, uint64_t seed, float* d_out, int64_t cap, int64_t* n_out,
                          void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_SYNTH] || !ctx->ready[RVCX_MODEL_HUBERT])
      throw Error(RVCX_E_STATE, "synthesizer/hubert not finalized");
    if (!d_audio || !d_out || n <= 0 || (ctx->scfg.f0 && (!d_pitch || !d_pitchf)))
      throw Error(RVCX_E_INVALID, "bad arguments");
    set_device(ctx);
    if (index_rate > 0 && !ctx->ivf) throw Error(RVCX_E_STATE, "index_rate > 0 but no feature index loaded");
    const int64_t no = vc_forward(*ctx, d_audio, n, d_pitch, d_pitchf, n / 160, sid, protect, index_rate, d_eps_z,
                                  d_eps_src, seed, d_out, cap, static_cast<hipStream_t>(stream));
    if (n_out) *n_out = no;
  });
}

int rvcx_set_highpass(rvcx_ctx* ctx, const double* b, const double* a, const double* zi, int order) {
  return guard(ctx, [&] {
    if (!b || !a || !zi) throw Error(RVCX_E_INVALID, "null coefficients");
    set_highpass(*ctx, b, a, zi, order);
  });
}

int rvcx_set_highpass_sos(rvcx_ctx* ctx, const double* sos, int nsec) {
  return guard(ctx, [&] {
    if (!sos) throw Error(RVCX_E_INVALID, "null sections");
    if (ctx->hp_order == 0) throw Error(RVCX_E_STATE, "set the (b, a) form first (rvcx_set_highpass)");
    set_device(ctx);
    set_highpass_sos(*ctx, sos, nsec);
  });
}

int rvcx_highpass_pad(rvcx_ctx* ctx, const double* d_audio, int64_t n, int64_t t_pad, double* d_pad64, float* d_pad32,
                      void* stream) {
  return guard(ctx, [&] {
    if (!d_audio || !d_pad32 || n <= 0 || t_pad < 0) throw Error(RVCX_E_INVALID, "rvcx_highpass_pad: bad arguments");
    set_device(ctx);
    highpass_pad(*ctx, d_audio, n, t_pad, d_pad64, d_pad32, static_cast<hipStream_t>(stream));
  });
}

// ceil(n*up/down) with up/down reduced; false when it does not fit an int64
static bool resample_len(int64_t n, int up, int down, int64_t* out) {
  const __int128 v = ((__int128)n * up + down - 1) / down;
  if (v > (__int128)INT64_MAX) return false;
  *out = (int64_t)v;
  return true;
}

static int gcd_int(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b, b = t;
  }
  return a;
}

int rvcx_resample_poly_len(int64_t n, int up, int down, int64_t* n_out) {
  if (!n_out || n < 0 || up < 1 || down < 1) return RVCX_E_INVALID;
  const int g = gcd_int(up, down);
  return resample_len(n, up / g, down / g, n_out) ? RVCX_OK : RVCX_E_INVALID;
}

int rvcx_resample_poly_v(rvcx_ctx* ctx, const void* d_x, int dtype, int channels, const int64_t* n, int64_t ldx, int B,
                         int up, int down, const double* d_taps, int64_t ntaps, double* d_y, int64_t ldy,
                         int64_t* n_out, void* stream) {
  return guard(ctx, [&] {
    if (!d_x || !n || !d_taps || !d_y || !n_out || B < 1 || B > 65535 || channels < 1 || channels > 65535 ||
        dtype < 0 || dtype > 3 || ldx < 1 || ldy < 1)
      throw Error(RVCX_E_INVALID, "rvcx_resample_poly_v: bad arguments");
    if (up < 1 || down < 1 || gcd_int(up, down) != 1)
      throw Error(RVCX_E_SHAPE, "rvcx_resample_poly_v: up and down must be positive and coprime");
    if (ntaps != 20 * (int64_t)std::max(up, down) + 1 && !(ntaps == 1 && up == 1 && down == 1))
      throw Error(RVCX_E_INVALID, "rvcx_resample_poly_v: ntaps must be 20*max(up, down) + 1 (or 1 for up == down == 1)");
    std::vector<long long> rows(2 * (size_t)B);
    for (int b = 0; b < B; ++b) {
      int64_t no = 0;
      if (n[b] < 1 || (B > 1 && n[b] > ldx) || !resample_len(n[b], up, down, &no))
        throw Error(RVCX_E_INVALID, "rvcx_resample_poly_v: bad row length");
      if (no > ldy) throw Error(RVCX_E_SHAPE, "rvcx_resample_poly_v: ldy below a row's output length");
      rows[b] = n[b], rows[(size_t)B + b] = no;
    }
    const ResamplePlan p = resample_poly_plan(up, down, ntaps);
    if (p.J < 1) throw Error(RVCX_E_SHAPE, "rvcx_resample_poly_v: ceil(ntaps / up) exceeds the staged input window");
    if ((ldy + p.J - 1) / p.J > INT32_MAX) throw Error(RVCX_E_SHAPE, "rvcx_resample_poly_v: ldy too large");
    set_device(ctx);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* hp = ctx->buf<double>("rs.taps", (size_t)up * p.K, st);
    long long* dr = ctx->buf<long long>("rs.rows", rows.size(), st);
    RVCX_HIP(hipMemcpyAsync(dr, rows.data(), sizeof(long long) * rows.size(), hipMemcpyHostToDevice, st));
    check(resample_poly_taps(d_taps, ntaps, up, p.K, hp, st), "resample_poly_taps");
    check(resample_poly_rows(p, d_x, dtype, channels, dr, ldx, B, up, down, hp, d_y, ldy, dr + B, st),
          "resample_poly_rows");
    for (int b = 0; b < B; ++b) n_out[b] = rows[(size_t)B + b];
  });
}

int rvcx_pipeline(rvcx_ctx* ctx, const double* d_audio, int64_t n, int sid, double semitones, float protect,
                  int64_t t_pad, int64_t t_pad_tgt, const float* d_eps_z, const float* d_eps_src, uint64_t seed,
                  float* d_out, int64_t cap, int64_t* n_out, double* d_f0, void* stream) {
  rvcx_pipeline_opts o = default_pipeline_opts();
  o.sid = sid;
  o.pitch = semitones;
  o.protect = protect;
  o.t_pad = t_pad;
  o.t_pad_tgt = t_pad_tgt;
  o.t_max = 0;  // single chunk
  return rvcx_pipeline_ex(ctx, d_audio, n, &o, d_eps_z, d_eps_src, seed, d_out, cap, n_out, d_f0, stream);
}

int rvcx_pipeline_default_opts(rvcx_pipeline_opts* opts) {
  if (!opts) return RVCX_E_INVALID;
  *opts = default_pipeline_opts();
  return RVCX_OK;
}

int rvcx_pipeline_ex(rvcx_ctx* ctx, const double* d_audio, int64_t n, const rvcx_pipeline_opts* opts,
                     const float* d_eps_z, const float* d_eps_src, uint64_t seed, float* d_out, int64_t cap,
                     int64_t* n_out, double* d_f0, void* stream) {
  return guard(ctx, [&] {
    if (!pipeline_ready(ctx)) throw Error(RVCX_E_STATE, "models not finalized");
    if (!d_audio || !d_out || !opts || n <= 0) throw Error(RVCX_E_INVALID, "bad arguments");
    set_device(ctx);
    const int64_t no = pipeline_forward_ex(*ctx, d_audio, n, *opts, d_eps_z, d_eps_src, seed, d_out, cap, d_f0,
                                           static_cast<hipStream_t>(stream), false);
    if (n_out) *n_out = no;
  });
}

int rvcx_set_workspace(rvcx_ctx* ctx, void* d_base, int64_t bytes) {
  return guard(ctx, [&] {
    if ((d_base && bytes <= 0) || (!d_base && bytes != 0) || (reinterpret_cast<uintptr_t>(d_base) & 255))
      throw Error(RVCX_E_INVALID, "rvcx_set_workspace: a 256-B aligned base with bytes > 0, or NULL and 0");
    set_device(ctx);
    ctx->release_pool();
    ctx->arena = static_cast<char*>(d_base);
    ctx->arena_bytes = d_base ? (size_t)bytes : 0;
  });
}

int rvcx_workspace_info(const rvcx_ctx* ctx, int64_t* held, int64_t* arena_bytes, int64_t* arena_used) {
  if (!ctx) return RVCX_E_INVALID;
  if (held) *held = (int64_t)ctx->pool_bytes();
  if (arena_bytes) *arena_bytes = (int64_t)ctx->arena_bytes;
  if (arena_used) *arena_used = (int64_t)ctx->arena_used;
  return RVCX_OK;
}

int rvcx_workspace_bytes(rvcx_ctx* ctx, int B, int64_t n, const rvcx_pipeline_opts* opts, int64_t* bytes,
                         void* stream) {
  return guard(ctx, [&] {
    if (!pipeline_ready(ctx)) throw Error(RVCX_E_STATE, "models not finalized");
    if (!opts || !bytes || n <= 0 || B < 1) throw Error(RVCX_E_INVALID, "rvcx_workspace_bytes: bad arguments");
    set_device(ctx);
    *bytes = pipeline_workspace_bytes(*ctx, B, n, *opts, static_cast<hipStream_t>(stream));
  });
}

int rvcx_device_status(rvcx_ctx* ctx, void* stream) {
  return guard(ctx, [&] {
    RVCX_HIP(hipSetDevice(ctx->device));
    RVCX_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    if (ctx->aux) RVCX_HIP(hipStreamSynchronize(ctx->aux));
    ctx->check_device_status();
  });
}

int rvcx_index_parse(const void* bytes, int64_t nbytes, int64_t* d, int64_t* ntotal, int64_t* nlist,
                     int64_t* nprobe, char* err, int64_t err_cap) {
  try {
    if (!bytes || nbytes <= 0) throw Error(RVCX_E_INVALID, "index_parse: empty buffer");
    const ParsedIvf P = parse_ivf(static_cast<const uint8_t*>(bytes), nbytes);
    if (d) *d = P.d;
    if (ntotal) *ntotal = P.ntotal;
    if (nlist) *nlist = P.nlist;
    if (nprobe) *nprobe = P.nprobe;
    if (err && err_cap > 0) err[0] = 0;
    return RVCX_OK;
  } catch (const Error& e) {
    if (err && err_cap > 0) std::snprintf(err, (size_t)err_cap, "%s", e.what());
    return e.code;
  } catch (const std::exception& e) {
    if (err && err_cap > 0) std::snprintf(err, (size_t)err_cap, "%s", e.what());
    return RVCX_E_INVALID;
  }
}

int rvcx_config_info(const rvcx_ctx* ctx, char* buf, int64_t cap, int64_t* len) {
  // JSON: the effective contraction arithmetic, the developer-knob opt-in and every RVCX_* variable of the process
  // environment with whether it is honoured (ctx may be NULL: the process-wide part only, no device needed)
  std::string j = "{\"arch\": \"gfx950\"";
  if (ctx) j += ", \"conv_math_ctx\": " + std::to_string(ctx->conv_math);
  const char* cm = rvcx_knob("RVCX_CONV_MATH");
  j += ", \"conv_math_default\": \"" + std::string(cm ? cm : "h16") + "\"";
  j += ", \"experimental\": " + std::string(experimental_on() ? "true" : "false");
  if (ctx) j += ", \"arena_bytes\": " + std::to_string(ctx->arena_bytes);
  if (ctx) j += ", \"dec_window\": " + std::string(ctx->dec_window ? "true" : "false");
  j += ", \"env\": {";
  bool first = true;
  for (char** e = environ; e && *e; ++e) {
    if (std::strncmp(*e, "RVCX_", 5) != 0) continue;
    const char* eq = std::strchr(*e, '=');
    if (!eq) continue;
    std::string k(*e, eq - *e), v(eq + 1);
    std::string ve;
    for (char ch : v)
      if (ch != '"' && ch != '\\' && (unsigned char)ch >= 32) ve += ch;
    const bool honoured = k == "RVCX_EXPERIMENTAL" || k == "RVCX_PROF_DUMP" || k == "RVCX_LIB" || experimental_on();
    j += std::string(first ? "" : ", ") + "\"" + k + "\": {\"value\": \"" + ve + "\", \"honoured\": " +
         (honoured ? "true" : "false") + "}";
    first = false;
  }
  j += "}}";
  if (len) *len = (int64_t)j.size();
  if (buf && cap > 0) {
    const size_t n = std::min<size_t>(j.size(), (size_t)cap - 1);
    std::memcpy(buf, j.data(), n);
    buf[n] = 0;
  }
  return (int64_t)j.size() < cap || !buf ? RVCX_OK : RVCX_E_CAPACITY;
}

int rvcx_profile(rvcx_ctx* ctx, int enable) {
  return guard(ctx, [&] { ctx->prof = enable != 0; });
}

int rvcx_profile_read(rvcx_ctx* ctx, double* total_ms, double* total_flops, int64_t* launches) {
  return rvcx_profile_read_ex(ctx, total_ms, total_flops, launches, nullptr);
}

int rvcx_profile_read_ex(rvcx_ctx* ctx, double* total_ms, double* total_flops, int64_t* launches, double* ceiling_ms) {
  return rvcx_profile_read_kinds(ctx, total_ms, total_flops, launches, ceiling_ms, 0, nullptr, nullptr, nullptr,
                                 nullptr, nullptr);
}

const char* rvcx_profile_kind_name(int kind) { return (kind >= 0 && kind < CK_COUNT) ? conv_kind_name(kind) : nullptr; }

int rvcx_profile_read_kinds(rvcx_ctx* ctx, double* total_ms, double* total_flops, int64_t* launches, double* ceiling_ms,
                            int nk, double* k_ms, double* k_flops, double* k_ceiling_ms, double* k_bytes,
                            int64_t* k_launches) {
  return guard(ctx, [&] {
    if (nk < 0 || (nk > 0 && (!k_ms || !k_flops || !k_ceiling_ms || !k_bytes || !k_launches)))
      throw Error(RVCX_E_INVALID, "profile_read_kinds: nk > 0 needs all five per-kind arrays");
    set_device(ctx);
    for (int k = 0; k < nk; ++k) k_ms[k] = k_flops[k] = k_ceiling_ms[k] = k_bytes[k] = 0.0, k_launches[k] = 0;
    double ms = 0.0, fl = 0.0, cms = 0.0;
    const char* dump = std::getenv("RVCX_PROF_DUMP");  // append one CSV line per conv launch
    FILE* fd = dump ? std::fopen(dump, "a") : nullptr;
    for (auto& r : ctx->prof_recs) {
      RVCX_HIP(hipEventSynchronize(r.b));
      float t = 0.f;
      RVCX_HIP(hipEventElapsedTime(&t, r.a, r.b));
      if (fd)
        std::fprintf(fd, "%d,%d,%d,%d,%d,%d,%d,%.6f,%.0f,%.0f,%.1f\n", r.two_d, r.M, r.N, r.C_in, r.taps, r.batch, r.ksplit,
                     t, r.flops, r.bytes, r.peak_tf);
      ms += t;
      fl += r.flops;
      cms += r.flops / (r.peak_tf * 1e9);
      if (r.kind >= 0 && r.kind < nk) {
        k_ms[r.kind] += t;
        k_flops[r.kind] += r.flops;
        k_ceiling_ms[r.kind] += r.flops / (r.peak_tf * 1e9);
        k_bytes[r.kind] += r.bytes;
        k_launches[r.kind] += 1;
      }
      ctx->prof_pool.push_back(r.a);
      ctx->prof_pool.push_back(r.b);
    }
    if (fd) std::fclose(fd);
    if (total_ms) *total_ms = ms;
    if (total_flops) *total_flops = fl;
    if (launches) *launches = (int64_t)ctx->prof_recs.size();
    if (ceiling_ms) *ceiling_ms = cms;
    ctx->prof_recs.clear();
  });
}

// ------------------------------------------------------------------ feature index (FAISS IVFFlat)
int rvcx_index_load(rvcx_ctx* ctx, const void* bytes, int64_t nbytes) {
  return guard(ctx, [&] {
    if (!bytes || nbytes <= 0) throw Error(RVCX_E_INVALID, "index_load: empty buffer");
    set_device(ctx);
    index_load(*ctx, static_cast<const uint8_t*>(bytes), nbytes);
  });
}

int rvcx_index_unload(rvcx_ctx* ctx) {
  return guard(ctx, [&] {
    set_device(ctx);
    RVCX_HIP(hipDeviceSynchronize());
    ctx->ivf.reset();
  });
}

int rvcx_index_info(const rvcx_ctx* ctx, int64_t* d, int64_t* ntotal, int64_t* nlist, int64_t* nprobe) {
  if (!ctx) return RVCX_E_INVALID;
  if (!ctx->ivf) return RVCX_E_STATE;
  const IvfView& v = ctx->ivf->view;
  if (d) *d = v.d;
  if (ntotal) *ntotal = v.ntotal;
  if (nlist) *nlist = v.nlist;
  if (nprobe) *nprobe = v.nprobe;
  return RVCX_OK;
}

int rvcx_index_set_nprobe(rvcx_ctx* ctx, int64_t nprobe) {
  return guard(ctx, [&] {
    if (!ctx->ivf) throw Error(RVCX_E_STATE, "no feature index loaded");
    if (nprobe < 1) throw Error(RVCX_E_INVALID, "nprobe must be >= 1");
    ctx->ivf->view.nprobe = (int)std::min<int64_t>(nprobe, ctx->ivf->view.nlist);
  });
}

int rvcx_index_search(rvcx_ctx* ctx, const float* d_x, int64_t n, int k, float* d_dist, int64_t* d_ids,
                      void* stream) {
  return guard(ctx, [&] {
    if ((!d_x && n > 0) || !d_dist || !d_ids || n < 0) throw Error(RVCX_E_INVALID, "index_search: bad arguments");
    set_device(ctx);
    index_search(*ctx, d_x, n, k, d_dist, d_ids, static_cast<hipStream_t>(stream));
  });
}

int rvcx_index_reconstruct_n(rvcx_ctx* ctx, int64_t i0, int64_t ni, float* d_out, void* stream) {
  return guard(ctx, [&] {
    if (!d_out && ni > 0) throw Error(RVCX_E_INVALID, "reconstruct_n: null output");
    set_device(ctx);
    index_reconstruct_n(*ctx, i0, ni, d_out, static_cast<hipStream_t>(stream));
  });
}

int rvcx_index_retrieve(rvcx_ctx* ctx, const float* d_feats, int64_t L, int d, double index_rate, float* d_out,
                        void* stream) {
  return guard(ctx, [&] {
    if ((!d_feats || !d_out) && L > 0) throw Error(RVCX_E_INVALID, "index_retrieve: bad arguments");
    set_device(ctx);
    index_retrieve(*ctx, d_feats, L, d, index_rate, d_out, static_cast<hipStream_t>(stream));
  });
}

int rvcx_index_default_build_opts(rvcx_index_build_opts* o) {
  if (!o) return RVCX_E_INVALID;
  o->niter = 10;
  o->nprobe = 1;
  o->seed = 0;
  o->init_rows = nullptr;
  return RVCX_OK;
}

int rvcx_index_build(rvcx_ctx* ctx, const float* d_x, int64_t n, int d, int64_t nlist,
                     const rvcx_index_build_opts* opts, void* stream) {
  return guard(ctx, [&] {
    rvcx_index_build_opts o;
    rvcx_index_default_build_opts(&o);
    if (opts) o = *opts;
    set_device(ctx);
    index_build(*ctx, d_x, n, d, nlist, o, static_cast<hipStream_t>(stream));
  });
}

int rvcx_index_centroids(rvcx_ctx* ctx, float* d_out, void* stream) {
  return guard(ctx, [&] {
    if (!d_out) throw Error(RVCX_E_INVALID, "index_centroids: null output");
    set_device(ctx);
    index_centroids(*ctx, d_out, static_cast<hipStream_t>(stream));
  });
}

int rvcx_index_save(rvcx_ctx* ctx, void* bytes, int64_t cap, int64_t* nbytes) {
  return guard(ctx, [&] {
    const int64_t nb = index_save(*ctx, bytes, cap);
    if (nbytes) *nbytes = nb;
  });
}

// ------------------------------------------------------------------ streaming (C5)
int rvcx_rt_default_desc(rvcx_rt_desc* d) {
  if (!d) return RVCX_E_INVALID;
  d->n_streams = 1;
  d->read_chunk_size = 192;  // rvc/realtime/callbacks.py:16-18
  d->cross_fade_overlap_size = 0.1;
  d->extra_convert_size = 0.5;
  d->silent_threshold = -90.0;
  d->f0_method = 0;
  d->fcpe_threshold = FCPE_THRESHOLD;
  return RVCX_OK;
}

int rvcx_rt_default_opts(rvcx_rt_opts* o) {
  if (!o) return RVCX_E_INVALID;
  std::memset(o, 0, sizeof(*o));
  o->index_rate = 0.0;
  o->protect = 0.5f;
  o->volume_envelope = 1.0;
  o->f0_autotune_strength = 1.0;
  o->proposed_pitch_threshold = 155.0;
  return RVCX_OK;
}

int rvcx_spectral_gate(rvcx_ctx* ctx, const float* d_x, int B, int64_t n, int64_t ldx, int sr, const float* strength,
                       float* d_y, int64_t ldy, uint8_t* d_mask, void* stream) {
  return guard(ctx, [&] {
    if (!d_x || !d_y || !strength || B < 1 || B > 65535 || n < 0 || ldx < n || ldy < n)
      throw Error(RVCX_E_INVALID, "spectral_gate: bad arguments");
    spectral_gate_check(n, sr);
    std::vector<float> p((size_t)B);
    for (int b = 0; b < B; ++b) {
      if (!(strength[b] <= 1.f)) throw Error(RVCX_E_INVALID, "spectral_gate: strength above 1 (or NaN)");
      p[b] = strength[b] < 0.f ? -1.f : strength[b];
    }
    set_device(ctx);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* dp = ctx->buf<float>("sg.strength", (size_t)B, st);
    RVCX_HIP(hipMemcpyAsync(dp, p.data(), sizeof(float) * (size_t)B, hipMemcpyHostToDevice, st));
    spectral_gate_run(*ctx, d_x, B, n, ldx, sr, dp, d_y, ldy, d_mask, st);
  });
}

int rvcx_rt_set_clean(rvcx_ctx* ctx, rvcx_rt* rt, int stream_index, int clean_audio, double clean_strength) {
  return guard(ctx, [&] {
    if (!rt || !rt->s) throw Error(RVCX_E_INVALID, "rt_set_clean: null stream group");
    rt_set_clean(*ctx, *rt->s, stream_index, clean_audio, clean_strength);
  });
}

int rvcx_rt_create(rvcx_ctx* ctx, const rvcx_rt_desc* desc, rvcx_rt** out) {
  return guard(ctx, [&] {
    if (!desc || !out) throw Error(RVCX_E_INVALID, "rt_create: null argument");
    set_device(ctx);
    auto* h = new rvcx_rt();
    try {
      h->s = rt_create(*ctx, *desc);
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
  });
}

int rvcx_rt_destroy(rvcx_ctx* ctx, rvcx_rt* rt) {
  return guard(ctx, [&] {
    if (!rt) return;
    set_device(ctx);
    RVCX_HIP(hipDeviceSynchronize());
    rt_destroy(rt->s);
    delete rt;
  });
}

int rvcx_rt_geometry(const rvcx_rt* rt, int64_t* g) {
  if (!rt || !rt->s || !g) return RVCX_E_INVALID;
  rt_geometry(*rt->s, g);
  return RVCX_OK;
}

int rvcx_rt_reset(rvcx_ctx* ctx, rvcx_rt* rt, void* stream) {
  return guard(ctx, [&] {
    if (!rt || !rt->s) throw Error(RVCX_E_INVALID, "rt_reset: null stream group");
    set_device(ctx);
    rt_reset(*ctx, *rt->s, static_cast<hipStream_t>(stream));
  });
}

int rvcx_rt_reset_stream(rvcx_ctx* ctx, rvcx_rt* rt, int stream_index, void* stream) {
  return guard(ctx, [&] {
    if (!rt || !rt->s) throw Error(RVCX_E_INVALID, "rt_reset_stream: null stream group");
    set_device(ctx);
    rt_reset_stream(*ctx, *rt->s, stream_index, static_cast<hipStream_t>(stream));
  });
}

int rvcx_rt_process_v(rvcx_ctx* ctx, rvcx_rt* rt, const float* d_in, const int32_t* sids, const rvcx_rt_opts* opts,
                      const uint8_t* active, const float* d_eps_z, const float* d_eps_src, uint64_t seed,
                      float* d_out, float* d_vol, int32_t* d_offs, void* stream) {
  return guard(ctx, [&] {
    if (!rt || !rt->s || !d_in || !sids || !opts || !d_out) throw Error(RVCX_E_INVALID, "rt_process_v: null argument");
    set_device(ctx);
    rt_process(*ctx, *rt->s, d_in, sids, opts, active, d_eps_z, d_eps_src, seed, d_out, d_vol, d_offs,
               static_cast<hipStream_t>(stream));
  });
}

// one rvcx_rt_opts for the whole group: rvcx_rt_process_v with B copies of it and every slot active
int rvcx_rt_process(rvcx_ctx* ctx, rvcx_rt* rt, const float* d_in, const int32_t* sids, const rvcx_rt_opts* opts,
                    const float* d_eps_z, const float* d_eps_src, uint64_t seed, float* d_out, float* d_vol,
                    int32_t* d_offs, void* stream) {
  if (!rt || !rt->s || !opts) return rvcx_rt_process_v(ctx, rt, d_in, sids, nullptr, nullptr, d_eps_z, d_eps_src, seed,
                                                       d_out, d_vol, d_offs, stream);
  const std::vector<rvcx_rt_opts> each((size_t)rt_streams(*rt->s), *opts);
  return rvcx_rt_process_v(ctx, rt, d_in, sids, each.data(), nullptr, d_eps_z, d_eps_src, seed, d_out, d_vol, d_offs,
                           stream);
}

// ------------------------------------------------------------------ batched offline conversion (C4)
int rvcx_pipeline_batch(rvcx_ctx* ctx, const double* d_audio, int64_t n, int64_t lda, int B,
                        const rvcx_pipeline_opts* opts, const int32_t* sids, const float* d_eps_z,
                        const float* d_eps_src, uint64_t seed, float* d_out, int64_t ldo, int64_t* n_out,
                        double* d_f0, float* d_hidden, void* stream) {
  return guard(ctx, [&] {
    if (!pipeline_ready(ctx)) throw Error(RVCX_E_STATE, "models not finalized");
    if (!d_audio || !opts || !sids || !d_out || n <= 0 || B < 1 || lda < n)
      throw Error(RVCX_E_INVALID, "rvcx_pipeline_batch: bad arguments");
    set_device(ctx);
    if (d_hidden && (opts->f0_method != 0 || !ctx->scfg.f0))
      throw Error(RVCX_E_INVALID, "rvcx_pipeline_batch: d_hidden needs the RMVPE f0 method and a pitch-guided model");
    const int64_t no = pipeline_forward_batch(*ctx, d_audio, n, lda, B, *opts, sids, d_eps_z, d_eps_src, seed, d_out,
                                              ldo, d_f0, d_hidden, static_cast<hipStream_t>(stream));
    if (n_out) *n_out = no;
  });
}

int rvcx_pipeline_batch_v(rvcx_ctx* ctx, const double* d_audio, const int64_t* n, int64_t lda, int B,
                          const rvcx_pipeline_opts* opts, const int32_t* sids, const float* d_eps_z,
                          const float* d_eps_src, uint64_t seed, float* d_out, int64_t ldo, int64_t* n_out,
                          double* d_f0, int64_t ldf, void* stream) {
  return rvcx_pipeline_batch_voices(ctx, d_audio, n, lda, B, opts, sids, nullptr, d_eps_z, d_eps_src, seed, d_out, ldo,
                                    n_out, d_f0, ldf, stream);
}

int rvcx_pipeline_batch_voices(rvcx_ctx* ctx, const double* d_audio, const int64_t* n, int64_t lda, int B,
                               const rvcx_pipeline_opts* opts, const int32_t* sids, const int32_t* voices,
                               const float* d_eps_z, const float* d_eps_src, uint64_t seed, float* d_out, int64_t ldo,
                               int64_t* n_out, double* d_f0, int64_t ldf, void* stream) {
  return guard(ctx, [&] {
    // the current voice's synthesizer when no voices are given; each row's voice is checked by the rows themselves
    if (!(voices ? ctx->ready[RVCX_MODEL_HUBERT] && ctx->ready[RVCX_MODEL_RMVPE] : pipeline_ready(ctx)))
      throw Error(RVCX_E_STATE, "models not finalized");
    if (!d_audio || !n || !opts || !sids || !d_out || !n_out || B < 1)
      throw Error(RVCX_E_INVALID, "rvcx_pipeline_batch_v: bad arguments");
    set_device(ctx);
    pipeline_forward_rows(*ctx, d_audio, n, lda, B, *opts, sids, d_eps_z, d_eps_src, seed, d_out, ldo, n_out, d_f0, ldf,
                          nullptr, static_cast<hipStream_t>(stream), false, voices);
  });
}

}  // extern "C"
