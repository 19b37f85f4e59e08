// extern "C" boundary (include/rvcx.h). Every entry point converts C++ exceptions into an
// rvcx_status and stores the message for rvcx_last_error.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

#include "../../include/rvcx_test.h"
#include "runtime.h"

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

struct rvcx_ctx : public Ctx {};
struct rvcx_rt {
  RtState* s = nullptr;
};

namespace {

template <class F>
int guard(rvcx_ctx* c, F&& f) {
  if (!c) return RVCX_E_INVALID;
  try {
    c->err.clear();
    f();
    return RVCX_OK;
  } catch (const Error& e) {
    c->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    c->err = e.what();
    return RVCX_E_INVALID;
  }
}

// every compute entry point: select the device and report device-side faults of earlier, completed calls
void set_device(rvcx_ctx* c) {
  RVCX_HIP(hipSetDevice(c->device));
  c->check_device_status();
  c->begin_call();
}

}  // namespace

namespace {
// the synthesizer configuration a descriptor names (rvcx_set_synth_config, rvcx_dec_margin_frames)
SynthCfg synth_cfg_of(const rvcx_synth_desc* d) {
  if (!d) throw Error(RVCX_E_INVALID, "null desc");
  SynthCfg g;
  g.I = d->inter_channels;
  g.H = d->hidden_channels;
  g.F = d->filter_channels;
  g.n_heads = d->n_heads;
  g.n_layers = d->n_layers;
  g.ksize = d->kernel_size;
  if (d->n_resblocks < 1 || d->n_resblocks > 4 || d->n_dilations < 1 || d->n_dilations > 4)
    throw Error(RVCX_E_INVALID, "resblock config out of range");
  g.rb_k.assign(d->resblock_kernel_sizes, d->resblock_kernel_sizes + d->n_resblocks);
  g.rb_d.clear();
  for (int j = 0; j < d->n_resblocks; ++j)
    g.rb_d.emplace_back(d->resblock_dilation_sizes[j], d->resblock_dilation_sizes[j] + d->n_dilations);
  if (d->n_upsample < 1 || d->n_upsample > 8) throw Error(RVCX_E_INVALID, "n_upsample out of range");
  g.ups.assign(d->upsample_rates, d->upsample_rates + d->n_upsample);
  g.up_k.assign(d->upsample_kernel_sizes, d->upsample_kernel_sizes + d->n_upsample);
  g.C0 = d->upsample_initial_channel;
  g.n_spk = d->spk_embed_dim;
  g.gin = d->gin_channels;
  g.sr = d->sr;
  g.emb_dim = d->text_enc_hidden_dim;
  g.f0 = d->no_f0 == 0;
  g.vocoder = d->vocoder;
  if (g.vocoder < 0 || g.vocoder > 2) throw Error(RVCX_E_INVALID, "unsupported vocoder id");
  if (!g.f0 && g.vocoder != 0)
    throw Error(RVCX_E_INVALID, "models without pitch guidance use the HiFi-GAN decoder only (synthesizers.py:119-139)");
  if (g.H % g.n_heads || g.I % 2 || g.C0 % (1 << g.ups.size()))
    throw Error(RVCX_E_INVALID, "inconsistent synthesizer dimensions");
  return g;
}

// the dispatcher's record of a 1-D test descriptor (rvcx_conv1d_ex, rvcx_conv_plan)
ConvArgs conv_args_of(const rvcx_conv_test_desc* d) {
  ConvArgs a;
  a.x = d->x; a.x_bs = d->x_bs; a.x_bs2 = d->x_bs2; a.ldx = d->ldx; a.T_in = d->T_in; a.C_in = d->C_in;
  a.pre_act = d->pre_act; a.pre_slope = d->pre_slope; a.pre_mask = d->pre_mask; a.pre_mask_bs = d->pre_mask_bs;
  a.w = d->w; a.ldw = d->C_in; a.w_ts = (long long)d->N * d->C_in; a.w_bs2 = d->w_bs2;
  a.taps = d->taps; a.stride = d->stride; a.dil = d->dil; a.pad = d->pad;
  a.y = d->y; a.y_bs = d->y_bs; a.y_bs2 = d->y_bs2; a.ldy = d->ldy; a.T_out = d->T_out; a.N = d->N;
  a.bias = d->bias; a.bias_bs2 = d->bias_bs2; a.alpha = d->alpha; a.act = d->act; a.slope = d->slope;
  a.res = d->res; a.res_bs = d->res_bs; a.res_bs2 = d->res_bs2; a.ldr = d->ldr; a.res_mode = d->res_mode;
  a.mask = d->mask; a.mask_bs = d->mask_bs; a.acc_mode = d->acc_mode; a.acc_div = d->acc_div;
  a.gate_h = d->gate_h; a.gate_g = d->gate_g; a.gate_g_bs = d->gate_g_bs;
  a.ln_g = d->ln_g; a.ln_b = d->ln_b; a.ln_eps = d->ln_eps;
  a.batch = d->batch; a.batch_inner = d->batch_inner;
  a.nz_har = d->nz_har; a.nz_bs = d->nz_bs; a.nz_stride = d->nz_stride; a.nz_kk = d->nz_kk; a.nz_u = d->nz_u;
  a.nz_C = d->nz_C; a.nz_w = d->nz_w; a.nz_b = d->nz_b;
  a.no_splitk = d->no_splitk ? 1 : 0;
  return a;
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
    ctx->ready[0] = false;
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
    if (model == RVCX_MODEL_SYNTH) {
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

int rvcx_hubert(rvcx_ctx* ctx, const float* d_audio, int64_t n, int version, float* d_feats, int64_t cap_rows,
                int64_t* rows_out, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[1]) throw Error(RVCX_E_STATE, "hubert weights not finalized");
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
    if (!ctx->ready[2]) throw Error(RVCX_E_STATE, "rmvpe weights not finalized");
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

int rvcx_fcpe_mel(rvcx_ctx* ctx, const float* d_audio, int64_t n, float* d_mel, int64_t cap_frames, int64_t* frames_out,
                  void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[RVCX_MODEL_FCPE]) throw Error(RVCX_E_STATE, "fcpe weights not finalized");
    if (!d_audio || !d_mel || n <= 0) throw Error(RVCX_E_INVALID, "rvcx_fcpe_mel: bad arguments");
    if (cap_frames < fcpe_frames(*ctx, n)) throw Error(RVCX_E_CAPACITY, "rvcx_fcpe_mel: output capacity too small");
    set_device(ctx);
    const int F = fcpe_mel(*ctx, d_audio, n, n, 1, d_mel, static_cast<hipStream_t>(stream));
    if (frames_out) *frames_out = F;
  });
}

int rvcx_performer_attention(rvcx_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, int H, int T,
                             const float* d_P, int M, float* d_out, void* stream) {
  return guard(ctx, [&] {
    if (!d_q || !d_k || !d_v || !d_P || !d_out || H <= 0 || T <= 0 || M <= 0)
      throw Error(RVCX_E_INVALID, "rvcx_performer_attention: bad argument");
    if (M > PERFORMER_MAX_FEATURES || (long long)H * T * 64 > INT32_MAX)
      throw Error(RVCX_E_SHAPE, "rvcx_performer_attention: at most 512 features and 2^31 elements per operand");
    set_device(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = ctx->buf<float>("perf.test.ws", (size_t)performer_ws_floats(H, T, M), s);
    check(performer_attention(d_q, d_k, d_v, (long long)T * 64, 64, H, T, d_P, M, ws, d_out, (long long)T * 64, 64, s),
          "performer_attention");
  });
}

int rvcx_performer_attention_b(rvcx_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, int B, int H, int T,
                               const float* d_P, int M, float* d_out, void* stream) {
  return guard(ctx, [&] {
    if (!d_q || !d_k || !d_v || !d_P || !d_out || B <= 0 || H <= 0 || T <= 0 || M <= 0)
      throw Error(RVCX_E_INVALID, "rvcx_performer_attention_b: bad argument");
    if (M > PERFORMER_MAX_FEATURES || B > 4096 || (long long)B * H * T * 64 > INT32_MAX)
      throw Error(RVCX_E_SHAPE, "rvcx_performer_attention_b: at most 512 features and 2^31 elements per operand");
    set_device(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = ctx->buf<float>("perf.test.ws", (size_t)performer_ws_floats(H, T, M, B), s);
    const long long bs = (long long)H * T * 64;
    check(performer_attention(d_q, d_k, d_v, (long long)T * 64, 64, H, T, d_P, M, ws, d_out, (long long)T * 64, 64, s, B,
                              bs, bs),
          "performer_attention");
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
    if (!ctx->ready[1]) throw Error(RVCX_E_STATE, "hubert weights not finalized");
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
    if (!ctx->ready[1]) throw Error(RVCX_E_STATE, "hubert weights not finalized");
    if (!d_audio || !d_feats || !n || B < 1 || ld_rows < 1) throw Error(RVCX_E_INVALID, "rvcx_hubert_batch_v: bad arguments");
    for (int b = 0; b < B; ++b)
      if (n[b] <= 0 || (B > 1 && n[b] > lda)) throw Error(RVCX_E_INVALID, "rvcx_hubert_batch_v: bad row length");
    set_device(ctx);
    hubert_forward_v(*ctx, d_audio, n, lda, B, version == 1 ? 1 : 2, d_feats, ld_rows, L_out,
                     static_cast<hipStream_t>(stream));
  });
}

int rvcx_rmvpe_batch(rvcx_ctx* ctx, const float* d_audio, int64_t n, int64_t lda, int B, float thred, double* d_f0,
                     int64_t cap_frames, int64_t* frames_out, float* d_hidden, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[2]) throw Error(RVCX_E_STATE, "rmvpe weights not finalized");
    if (!d_audio || !d_f0 || n <= 0 || B < 1 || lda < n) throw Error(RVCX_E_INVALID, "rvcx_rmvpe_batch: bad arguments");
    set_device(ctx);
    const int64_t F = rmvpe_forward_b(*ctx, d_audio, n, lda, B, thred, d_f0, cap_frames, d_hidden,
                                      static_cast<hipStream_t>(stream));
    if (frames_out) *frames_out = F;
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
    if (!ctx->ready[0]) throw Error(RVCX_E_STATE, "synthesizer weights not finalized");
    if (B <= 0 || T <= 0 || !d_phone || !d_lengths || !d_sid || !d_out)
      throw Error(RVCX_E_INVALID, "rvcx_synth_infer: bad arguments");
    if (ctx->scfg.f0 && (!d_pitch || !d_pitchf))
      throw Error(RVCX_E_INVALID, "rvcx_synth_infer: a pitch-guided model needs pitch and pitchf");
    if (!ctx->scfg.f0) d_pitch = nullptr, d_pitchf = nullptr;  // Synthesizer.infer ignores them (:233-239)
    set_device(ctx);
    synth_forward(*ctx, B, T, d_phone, d_lengths, d_pitch, d_pitchf, d_sid, d_eps_z, d_eps_src, seed, d_out, d_zp,
                  d_z, static_cast<hipStream_t>(stream));
  });
}

int rvcx_synth_infer_ex(rvcx_ctx* ctx, int B, int T, const float* d_phone, const int32_t* d_lengths,
                        const int32_t* d_pitch, const float* d_pitchf, const int32_t* d_sid, double rate,
                        const float* d_eps_z, const float* d_eps_src, uint64_t seed, float* d_out, float* d_zp,
                        float* d_z, float* d_m_p, float* d_logs_p, int* t_out, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[0]) throw Error(RVCX_E_STATE, "synthesizer weights not finalized");
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
    synth_forward(*ctx, B, T, d_phone, d_lengths, d_pitch, d_pitchf, d_sid, d_eps_z, d_eps_src, seed, d_out, d_zp,
                  d_z, static_cast<hipStream_t>(stream), 0, head, d_m_p, d_logs_p);
    if (t_out) *t_out = T - head;
  });
}

int rvcx_dec_only(rvcx_ctx* ctx, int B, int T, const float* d_z, const float* d_f0, const int32_t* d_sid,
                  const float* d_eps_src, uint64_t seed, float* d_out, void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[0]) throw Error(RVCX_E_STATE, "synthesizer weights not finalized");
    if (B <= 0 || T <= 0 || !d_z || !d_sid || !d_out || (ctx->scfg.f0 && !d_f0))
      throw Error(RVCX_E_INVALID, "rvcx_dec_only: bad arguments");
    set_device(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int I = ctx->scfg.I;
    float* zt = ctx->buf<float>("dec_only.z", (size_t)B * T * I, s);
    check(transpose_bct_btc(d_z, zt, B, I, T, s), "transpose");
    float* g = ctx->buf<float>("dec_only.g", (size_t)B * ctx->scfg.gin, s);
    check(gather_rows(ctx->W("emb_g"), ctx->scfg.gin, d_sid, g, B, ctx->scfg.gin, s), "emb_g");
    dec_forward(*ctx, B, T, zt, nullptr, d_f0, g, d_eps_src, seed, d_out, s);
  });
}

int rvcx_voice_conversion(rvcx_ctx* ctx, const float* d_audio, int64_t n, const int32_t* d_pitch,
                          const float* d_pitchf, int sid, float protect, double index_rate, const float* d_eps_z,
                          const float* d_eps_src, uint64_t seed, float* d_out, int64_t cap, int64_t* n_out,
                          void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[0] || !ctx->ready[1]) throw Error(RVCX_E_STATE, "synthesizer/hubert not finalized");
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
    if (!ctx->ready[0] || !ctx->ready[1] || !ctx->ready[2]) throw Error(RVCX_E_STATE, "models not finalized");
    if (!d_audio || !d_out || !opts || n <= 0) throw Error(RVCX_E_INVALID, "bad arguments");
    set_device(ctx);
    const int64_t no = pipeline_forward_ex(*ctx, d_audio, n, *opts, d_eps_z, d_eps_src, seed, d_out, cap, d_f0,
                                           static_cast<hipStream_t>(stream));
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
    if (!ctx->ready[0] || !ctx->ready[1] || !ctx->ready[2]) throw Error(RVCX_E_STATE, "models not finalized");
    if (!opts || !bytes || n <= 0 || B < 1) throw Error(RVCX_E_INVALID, "rvcx_workspace_bytes: bad arguments");
    set_device(ctx);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    // the call itself on zero audio, from an empty internally allocated pool; the pool is released again after, and
    // a caller arena stays attached (its regions are carved anew by the next call)
    char* const arena = ctx->arena;
    const size_t arena_bytes = ctx->arena_bytes;
    ctx->release_pool();
    ctx->arena = nullptr;
    ctx->arena_bytes = 0;
    struct PlanScope {
      Ctx& c;
      ~PlanScope() { c.sizing_plan = false; }
    } plan_scope{*ctx};
    ctx->sizing_plan = true;
    DevBuf audio, out;
    const int64_t m = n + 2 * opts->t_pad;
    const int64_t cap = (m / 160 + (opts->t_center > 0 ? n / opts->t_center : 0) + 2) * ctx->scfg.upp();
    int64_t need = 0;
    try {
      RVCX_HIP(hipMalloc(&audio.p, sizeof(double) * (size_t)(B * n)));
      RVCX_HIP(hipMalloc(&out.p, sizeof(float) * (size_t)(B * cap)));
      RVCX_HIP(hipMemsetAsync(audio.p, 0, sizeof(double) * (size_t)(B * n), s));
      auto measure = [&](const rvcx_pipeline_opts& o) {
        if (B == 1) {
          pipeline_forward_ex(*ctx, static_cast<const double*>(audio.p), n, o, nullptr, nullptr, 0,
                              static_cast<float*>(out.p), cap, nullptr, s);
        } else {
          // B rows of n samples in the batched pipeline's sizing form (Ctx::sizing_plan): run as a ragged batch (masks,
          // the gathered RMVPE group and one single-row RMVPE forward), whose regions hold the equal-length routes too
          std::vector<int32_t> sids((size_t)B, o.sid);
          std::vector<int64_t> nv((size_t)B, n), no((size_t)B);
          pipeline_forward_rows(*ctx, static_cast<const double*>(audio.p), nv.data(), n, B, o, sids.data(), nullptr,
                                nullptr, 0, static_cast<float*>(out.p), cap, no.data(), nullptr, 0, nullptr, s);
        }
        RVCX_HIP(hipStreamSynchronize(s));
        int64_t carved = (int64_t)ctx->carved;
        if (B > 1) {
          // a ragged batch walks its rows' front ends in another order than the call above, and the split-K slab all
          // convs share is regrown whenever a later conv needs a larger one: room for one regrowth per row and stream
          for (const char* slab : {"conv.splitk", "conv.splitk.aux"})
            if (ctx->ws.count(slab) && ctx->ws[slab]) carved += (int64_t)B * (int64_t)ctx->ws[slab]->bytes;
        }
        return carved;
      };
      need = measure(*opts);
      if (opts->f0_method == 3) {
        // FCPE's scratch is carved in place of RMVPE's, which can be the larger: the size also holds the same call
        // with the default f0 method, so an arena sized for "fcpe" serves a caller that switches back
        rvcx_pipeline_opts o0 = *opts;
        o0.f0_method = 0;
        ctx->release_pool();
        need = std::max(need, measure(o0));
      }
      // the per-chunk HuBERT feature buffers (pl.hb<i>) sum to the same total over any split plan up to one row and
      // the 256-B rounding per chunk
      if (B == 1 && opts->t_max > 0 && n + 160 > opts->t_max && opts->t_center > 0) {
        const int64_t nts = n > opts->t_center ? (n - 1 - opts->t_center) / opts->t_center + 1 : 0;
        need += (nts + 1) * ((int64_t)ctx->scfg.emb_dim * 4 + 512);
      }
    } catch (...) {
      ctx->release_pool();
      ctx->arena = arena;
      ctx->arena_bytes = arena_bytes;
      throw;
    }
    ctx->release_pool();
    ctx->arena = arena;
    ctx->arena_bytes = arena_bytes;
    *bytes = need;
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

int rvcx_set_conv_math(rvcx_ctx* ctx, int mode) {
  return guard(ctx, [&] {
    if (mode < 0 || mode > 3) throw Error(RVCX_E_INVALID, "conv math mode must be 0, 1, 2 or 3");
    ctx->conv_math = mode;
  });
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

int rvcx_set_dec_window(rvcx_ctx* ctx, int on) {
  return guard(ctx, [&] { ctx->dec_window = on != 0; });
}

int rvcx_dec_margin_frames(const rvcx_synth_desc* d, int* frames) {
  try {
    if (!frames) return RVCX_E_INVALID;
    *frames = dec_margin_frames(synth_cfg_of(d));
    return RVCX_OK;
  } catch (const Error& e) {
    return e.code;
  } catch (...) {
    return RVCX_E_INVALID;
  }
}

int rvcx_conv_plan(const rvcx_conv_test_desc* d, const rvcx_conv_plan_form* f, int two_d, int static_weight, int math,
                   int plan_T, int force_kind, int force_tile, int* kind, int* tile, int* ksplit, int* wsplit_fmt) {
  if (!d || !kind || !tile || !ksplit || !wsplit_fmt || math < 0 || math > 3 || (two_d && !f)) return RVCX_E_INVALID;
  ConvArgs a = conv_args_of(d);
  a.math = math;
  a.plan_T = plan_T;
  if (f) {
    a.W_in = f->W_in; a.W_out = f->W_out; a.KH = f->KH; a.KW = f->KW; a.padh = f->padh; a.padw = f->padw;
    a.out_map = f->out_map; a.out_cv = f->out_cv; a.b_kn = f->b_kn; a.lowp = f->lowp;
    if (f->ldw > 0) a.ldw = f->ldw;
    if (f->w_ts > 0) a.w_ts = f->w_ts;
    a.w_bs = f->w_bs; a.bias_bs = f->bias_bs;
  }
  const ConvPlan p = conv_plan(a, two_d != 0, static_weight != 0, ConvForce{force_kind, force_tile});
  *kind = p.kind, *tile = p.tile, *ksplit = p.ksplit, *wsplit_fmt = p.wsplit_fmt;
  return RVCX_OK;
}

int rvcx_set_generator_precision(rvcx_ctx* ctx, int) {
  return guard(ctx, [&] {
    throw Error(RVCX_E_INVALID,
                "rvcx_set_generator_precision was removed: set rvcx_rt_opts.gen_precision per streaming hop instead");
  });
}

int rvcx_conv1d(rvcx_ctx* ctx, const float* d_x, int64_t T, int C_in, const float* d_w, const float* d_bias, int N,
                int taps, int dilation, int pad, int stride, int math, float* d_y, int64_t T_out, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    ctx->check_device_status();
    if (!d_x || !d_w || !d_y || T <= 0 || C_in <= 0 || N <= 0 || taps <= 0 || dilation <= 0 || stride <= 0 ||
        pad < 0 || T_out <= 0 || math < 0 || math > 7)
      throw Error(RVCX_E_INVALID, "rvcx_conv1d: bad argument");
    if ((T_out - 1) * stride + (int64_t)(taps - 1) * dilation + 1 > T + 2 * (int64_t)pad)
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d: T_out exceeds the padded input");
    if (T > INT32_MAX || T_out > INT32_MAX || (int64_t)taps * N * C_in > INT32_MAX)
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d: size out of range");
    ConvArgs a;
    a.x = d_x; a.ldx = C_in; a.T_in = (int)T; a.C_in = C_in;
    a.w = d_w; a.ldw = C_in; a.w_ts = (long long)N * C_in; a.taps = taps; a.dil = dilation; a.pad = pad;
    a.stride = stride;
    a.y = d_y; a.ldy = N; a.T_out = (int)T_out; a.N = N; a.bias = d_bias;
    // math -> the arithmetic, the forced family, the reduced-precision mode. 3 / 5 / 6: the weight-streamed kernel on
    // the tile the size policy picks, unsplit (5: the two-plane fp16 arithmetic, 6: its hi plane alone); 4 / 7: the
    // gather-streamed kernel, split-K by the size policy (7: fp16)
    static const struct { int math, kind, lowp; } route[8] = {{0, -1, 0}, {1, -1, 0}, {2, -1, 0}, {2, CK_WSB16, 0},
                                                              {2, CK_GS, 0}, {3, CK_WSB16, 0}, {3, CK_WSB16, 1}, {3, CK_GS, 0}};
    a.math = route[math].math;
    a.lowp = route[math].lowp;
    a.no_splitk = route[math].kind == CK_WSB16;
    const ConvForce force{route[math].kind};
    launch_conv_test(*ctx, a, false, force.kind >= 0, force, -1, "rvcx_conv1d", static_cast<hipStream_t>(stream));
  });
}

int rvcx_conv1d_gen(rvcx_ctx* ctx, const float* d_x, int64_t T, int C_in, const float* d_w, const float* d_bias,
                    int N, int taps, int dilation, int pad, int pre_act, float pre_slope, int act, float slope,
                    const float* d_res, int acc_mode, float acc_div, int kernel, float* d_y, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    ctx->check_device_status();
    if (!d_x || !d_w || !d_y || T <= 0 || C_in <= 0 || N <= 0 || taps <= 0 || dilation <= 0 || pad < 0 || act < 0 ||
        act > 1 || pre_act < 0 || pre_act > 1 || acc_mode < 0 || acc_mode > 2 || kernel < 0 || kernel > 2 || (d_res && d_res == d_x))
      throw Error(RVCX_E_INVALID, "rvcx_conv1d_gen: bad argument");
    const int64_t T_out = T + 2 * (int64_t)pad - (int64_t)(taps - 1) * dilation;
    if (T_out <= 0 || T > INT32_MAX || (int64_t)taps * N * C_in > INT32_MAX)
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d_gen: size out of range");
    ConvArgs a;
    a.x = d_x; a.ldx = C_in; a.T_in = (int)T; a.C_in = C_in;
    a.w = d_w; a.ldw = C_in; a.w_ts = (long long)N * C_in; a.taps = taps; a.dil = dilation; a.pad = pad;
    a.y = d_y; a.ldy = N; a.T_out = (int)T_out; a.N = N; a.bias = d_bias;
    a.pre_act = pre_act ? ACT_LRELU : ACT_NONE;
    a.pre_slope = pre_slope;
    a.act = act ? ACT_LRELU : ACT_NONE;
    a.slope = slope;
    if (d_res) {
      a.res = d_res;
      a.ldr = N;
      a.res_mode = RES_ADD_POST;
    }
    a.acc_mode = acc_mode == 0 ? ACC_STORE : (acc_mode == 1 ? ACC_ADD : ACC_ADD_DIV);
    a.acc_div = acc_div;
    a.math = 3;
    a.no_splitk = 1;
    if (!conv_wsb_eligible(a)) throw Error(RVCX_E_SHAPE, "rvcx_conv1d_gen: shape not eligible for the weight-streamed kernel");
    // 0: the size policy's route, 1: the weight-streamed tile the policy would pick, 2: the weight-stationary kernel
    const ConvForce force{kernel == 1 ? CK_WSB16 : (kernel == 2 ? CK_WST : -1)};
    launch_conv_test(*ctx, a, false, true, force, -1, "rvcx_conv1d_gen", static_cast<hipStream_t>(stream));
  });
}

int rvcx_conv1d_ex(rvcx_ctx* ctx, const rvcx_conv_test_desc* d, int* kind_out, int* ksplit_out, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    ctx->check_device_status();
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!d || !d->x || !d->w || !d->y || d->T_in <= 0 || d->C_in <= 0 || d->N <= 0 || d->taps <= 0 || d->dil <= 0 ||
        d->stride <= 0 || d->pad < 0 || d->T_out <= 0 || d->batch <= 0 || d->batch_inner <= 0 || d->ldx < d->C_in ||
        d->ldy < (d->gate_h > 0 ? d->gate_h : d->N) || d->pre_act < 0 || d->pre_act > ACT_LOGCLAMP || d->act < 0 ||
        d->act > ACT_LOGCLAMP || d->res_mode < RES_NONE || d->res_mode > RES_RSUB_POST || d->acc_mode < ACC_STORE ||
        d->acc_mode > ACC_ADD_DIV || (d->res_mode != RES_NONE && !d->res) || (d->res && d->ldr != 0 && d->ldr < d->N) ||
        d->route < 0 || d->route > 5 || d->gate_h < 0 || (d->gate_h > 0 && !d->gate_g) ||
        (d->ln_g && (!d->ln_b || !d->res)) ||
        (d->nz_har && (!d->nz_w || !d->nz_b || d->nz_C <= 0 || d->nz_u <= 0 || d->nz_stride <= 0)) ||
        ctx->is_weight(d->w))
      throw Error(RVCX_E_INVALID, "rvcx_conv1d_ex: bad argument");
    if ((int64_t)(d->T_out - 1) * d->stride + (int64_t)(d->taps - 1) * d->dil + 1 > d->T_in + 2 * (int64_t)d->pad)
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d_ex: T_out exceeds the padded input");
    if ((int64_t)d->taps * d->N * d->C_in > INT32_MAX) throw Error(RVCX_E_SHAPE, "rvcx_conv1d_ex: size out of range");
    ConvArgs a = conv_args_of(d);
    // the combine-time epilogues as their kernels take them (launch_splitk_reduce's conditions)
    if (a.ln_g && (a.N > 1024 || a.batch_inner != 1 || a.res_mode != RES_NONE || a.acc_mode != ACC_STORE || a.gate_h > 0))
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d_ex: the combine's LayerNorm takes N <= 1024, one group, no other residual");
    if (a.gate_h > 0 && (a.N != 2 * a.gate_h || a.batch_inner != 1 || a.act != ACT_NONE || a.alpha != 1.f || a.res ||
                         a.mask || a.acc_mode != ACC_STORE))
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d_ex: the combine's gate takes N = 2 gate_h and no other epilogue field");
    if (a.nz_har && (a.nz_kk != 1 || a.N != a.nz_u * a.nz_C || a.gate_h > 0 || a.ln_g))
      throw Error(RVCX_E_SHAPE, "rvcx_conv1d_ex: the fused noise conv takes one tap and N = nz_u nz_C");
    // route -> the arithmetic, a static weight, the forced family and the family the launch has to get
    static const struct { int math, stat, force, expect; } route[6] = {{0, 1, -1, -1},       {1, 0, -1, CK_GEMM},
                                                                       {2, 0, -1, CK_EMU},   {3, 1, CK_WSB16, -1},
                                                                       {3, 1, CK_GS, -1},    {3, 1, CK_WST, -1}};
    const auto& r = route[d->route];
    a.math = r.math;
    const ConvPlan p = launch_conv_test(*ctx, a, false, r.stat != 0, ConvForce{r.force}, r.expect, "rvcx_conv1d_ex", s);
    if (ksplit_out) *ksplit_out = p.ksplit;
    if (kind_out) *kind_out = p.kind;
  });
}

int rvcx_conv2d3x3(rvcx_ctx* ctx, const float* d_x, int H, int W, int C_in, const float* d_w, const float* d_bias,
                   int N, int act, int math, float* d_y, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    ctx->check_device_status();
    if (!d_x || !d_w || !d_y || H <= 0 || W <= 0 || C_in <= 0 || N <= 0 || act < 0 || act > 1 || math < 0 || math > 2)
      throw Error(RVCX_E_INVALID, "rvcx_conv2d3x3: bad argument");
    if ((int64_t)H * W * (C_in > N ? C_in : N) > INT32_MAX) throw Error(RVCX_E_SHAPE, "rvcx_conv2d3x3: size out of range");
    ConvArgs a;
    a.x = d_x; a.ldx = C_in; a.T_in = H; a.W_in = W; a.C_in = C_in;
    a.w = d_w; a.ldw = C_in; a.w_ts = (long long)N * C_in; a.taps = 9; a.KH = 3; a.KW = 3; a.padh = 1; a.padw = 1;
    a.y = d_y; a.ldy = N; a.T_out = H; a.W_out = W; a.N = N; a.bias = d_bias;
    a.act = act ? ACT_RELU : ACT_NONE;
    // math 2: the windowed gather-streamed kernel of the U-Net's deep levels in the two-plane fp16 split (64 x 64 tiles,
    // K split over workgroups by the size policy); else the policy for a weight that is not static (the 3x3
    // small-channel form reads a fresh fp16 image under the fp16-split arithmetic)
    static const struct { int math, kind; } route[3] = {{0, -1}, {1, -1}, {3, CK_GSW}};
    a.math = route[math].math;
    const ConvForce force{route[math].kind};
    if (math == 2 && !conv_gsw_eligible(a)) throw Error(RVCX_E_SHAPE, "rvcx_conv2d3x3: shape not eligible for the windowed kernel");
    launch_conv_test(*ctx, a, true, math == 2, force, -1, "rvcx_conv2d3x3", static_cast<hipStream_t>(stream));
  });
}

int rvcx_convtranspose2d_s2(rvcx_ctx* ctx, const float* d_x, int H, int W, int C_in, const float* d_w,
                            const float* d_bias, int N, int act, int math, float* d_y, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    ctx->check_device_status();
    if (!d_x || !d_w || !d_y || H <= 0 || W <= 0 || C_in <= 0 || N <= 0 || act < 0 || act > 1 || math < 0 || math > 1)
      throw Error(RVCX_E_INVALID, "rvcx_convtranspose2d_s2: bad argument");
    if ((int64_t)4 * H * W * (C_in > 4 * N ? C_in : 4 * N) > INT32_MAX)
      throw Error(RVCX_E_SHAPE, "rvcx_convtranspose2d_s2: size out of range");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the phase-conv weights (and its bias per virtual column) in test buffers, rebuilt every call
    float* wp = ctx->buf<float>("conv.test.upw", (size_t)16 * N * C_in, s);
    check(upconv_phase_pack(d_w, C_in, N, wp, s), "upconv_phase_pack");
    float* bp = nullptr;
    if (d_bias) {
      bp = ctx->buf<float>("conv.test.upb", (size_t)4 * N, s);
      for (int p = 0; p < 4; ++p)
        RVCX_HIP(hipMemcpyAsync(bp + (size_t)p * N, d_bias, sizeof(float) * N, hipMemcpyDeviceToDevice, s));
    }
    ConvArgs a;  // runtime_fe.cpp's decoder up-conv
    a.x = d_x; a.ldx = C_in; a.T_in = H; a.W_in = W; a.C_in = C_in;
    a.w = wp; a.ldw = C_in; a.w_ts = (long long)4 * N * C_in; a.taps = 4; a.KH = 2; a.KW = 2;
    a.y = d_y; a.ldy = N; a.T_out = H; a.W_out = W; a.N = 4 * N;
    a.out_map = OUT_UPSAMPLE2D;
    a.out_cv = N;
    a.bias = bp;
    a.act = act ? ACT_RELU : ACT_NONE;
    // math 0: the gather-streamed kernel the pipeline's policy routes the up-convs to (under a split arithmetic); 1: the
    // native fp32 kernel
    a.math = math == 1 ? 1 : 0;
    const ConvForce force{math == 0 && conv_math(ctx->conv_math) >= 2 ? CK_GS : -1};
    launch_conv_test(*ctx, a, true, force.kind >= 0, force, -1, "rvcx_convtranspose2d_s2", s);
  });
}

int rvcx_flash_attention(rvcx_ctx* ctx, const float* d_qkv, int B, int T, int n_heads, int dk, float qscale,
                         const float* d_rel_k, const float* d_rel_v, int window, const float* d_mask, float* d_out,
                         void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    ctx->check_device_status();
    if (!d_qkv || !d_out || B <= 0 || T <= 0 || n_heads <= 0 || (dk != 64 && dk != 96) || window < 0 ||
        (d_rel_k != nullptr) != (d_rel_v != nullptr))
      throw Error(RVCX_E_INVALID, "rvcx_flash_attention: bad argument");
    if ((long long)B * T * 3 * n_heads * dk > INT32_MAX) throw Error(RVCX_E_SHAPE, "rvcx_flash_attention: too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nsplit = flash_attn_splits(B, n_heads, T);
    float* po = ctx->buf<float>("att.test.o", (size_t)flash_attn_ws_floats(B, n_heads, T, dk, nsplit), s);
    float* pml = ctx->buf<float>("att.test.ml", (size_t)nsplit * B * n_heads * T * 2, s);
    check(flash_attn(d_qkv, 3 * n_heads * dk, B, T, n_heads, dk, qscale, d_rel_k, d_rel_v, window, d_mask, po, pml,
                     nsplit, d_out, n_heads * dk, s),
          "flash_attn");
  });
}

int rvcx_resblock_pair(rvcx_ctx* ctx, const float* d_x, int B, int64_t T, int C, const float* d_w1, const float* d_b1,
                       const float* d_w2, const float* d_b2, int k, int dilation, int acc_mode, float acc_div, int cfg,
                       float* d_y, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    ctx->check_device_status();
    if (!d_x || !d_y || !d_w1 || !d_w2 || !d_b1 || !d_b2 || B <= 0 || T <= 0 || acc_mode < 0 || acc_mode > 2 ||
        d_x == d_y || cfg < 0)
      throw Error(RVCX_E_INVALID, "rvcx_resblock_pair: bad argument");
    if (!rb_pair_fits(C, k, dilation) || T > INT32_MAX / C)
      throw Error(RVCX_E_SHAPE, "rvcx_resblock_pair: shape not supported by the fused kernel");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int fmt = (cfg >> 4) & 3;
    if (fmt > 2) throw Error(RVCX_E_INVALID, "rvcx_resblock_pair: arithmetic (cfg bits 4-5) must be 0, 1 or 2");
    cfg &= 15;
    const int wfmt = fmt ? RB_WF16 : RB_WBF16;
    // fresh split images every call (test entry: the weight pointers may be reused by the caller)
    void* w1s = ctx->buf<char>("rb.test.w1s", (size_t)rb_wsplit_bytes(C, k, wfmt), s);
    void* w2s = ctx->buf<char>("rb.test.w2s", (size_t)rb_wsplit_bytes(C, k, wfmt), s);
    check(rb_wsplit_build(d_w1, C, k, w1s, s, wfmt), "rb_wsplit_build");
    check(rb_wsplit_build(d_w2, C, k, w2s, s, wfmt), "rb_wsplit_build");
    RbPairArgs a;
    a.wfmt = wfmt;
    a.lowp = fmt == 2;
    a.x = d_x;
    a.x_bs = T * C;
    a.w1s = w1s;
    a.b1 = d_b1;
    a.w2s = w2s;
    a.b2 = d_b2;
    a.C = C;
    a.k = k;
    a.d = dilation;
    a.T = (int)T;
    a.B = B;
    a.y = d_y;
    a.y_bs = T * C;
    a.acc_mode = acc_mode;
    a.acc_div = acc_div;
    check(rb_pair(a, cfg, s), "rb_pair");
  });
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

}  // extern "C"

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

int rvcx_kmeans_assign(rvcx_ctx* ctx, const float* d_x, int64_t n, int d, const float* d_cent, int64_t nlist,
                       int32_t* d_assign, float* d_dist, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    kmeans_assign_run(*ctx, d_x, n, d, d_cent, nlist, d_assign, d_dist, static_cast<hipStream_t>(stream));
  });
}

int rvcx_kmeans_update(rvcx_ctx* ctx, const float* d_x, int64_t n, int d, const int32_t* d_assign, int64_t nlist,
                       float* d_cent, int64_t* d_sizes, void* stream) {
  return guard(ctx, [&] {
    set_device(ctx);
    kmeans_update_run(*ctx, d_x, n, d, d_assign, nlist, d_cent, d_sizes, static_cast<hipStream_t>(stream));
  });
}

int rvcx_gru_bidir(rvcx_ctx* ctx, const float* d_gi, int B, int T, const float* d_whh_f, const float* d_bhh_f,
                   const float* d_whh_b, const float* d_bhh_b, float* d_out, int64_t tag_start, void* stream) {
  return guard(ctx, [&] {
    // T: the kernel's 32-bit row offsets (t * 1536); the weights are read as float4
    if (!d_gi || !d_whh_f || !d_bhh_f || !d_whh_b || !d_bhh_b || !d_out || B < 1 || B > 65535 || T < 1 ||
        T > (1 << 20) || tag_start > (int64_t)UINT32_MAX || (reinterpret_cast<uintptr_t>(d_whh_f) & 15) ||
        (reinterpret_cast<uintptr_t>(d_whh_b) & 15))
      throw Error(RVCX_E_INVALID, "rvcx_gru_bidir: bad arguments");
    set_device(ctx);
    ctx->before_gru = nullptr;  // nothing is issued beside this launch
    gru_bidir_run(*ctx, d_gi, B, T, d_whh_f, d_bhh_f, d_whh_b, d_bhh_b, d_out, tag_start < 0 ? -1 : (long long)tag_start,
                  static_cast<hipStream_t>(stream));
  });
}

int rvcx_dec_source(rvcx_ctx* ctx, int B, int T, const float* d_f0, const float* d_eps_src, uint64_t seed, float* d_har,
                    void* stream) {
  return guard(ctx, [&] {
    if (!ctx->ready[0] || !ctx->scfg.f0 || ctx->scfg.vocoder == 2)
      throw Error(RVCX_E_STATE, "rvcx_dec_source: needs a finalized pitch-guided HiFi-GAN (NSF) or MRF synthesizer");
    if (B < 1 || T < 1 || !d_f0 || !d_har) throw Error(RVCX_E_INVALID, "rvcx_dec_source: bad arguments");
    set_device(ctx);
    dec_source_rows(*ctx, B, T, d_f0, d_eps_src, seed, d_har, static_cast<hipStream_t>(stream));
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
  d->fcpe_threshold = 0.006f;  // rvc/realtime/pipeline.py:155
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

int rvcx_rt_model_rows(rvcx_ctx* ctx, rvcx_rt* rt, int gated, float* d_dst, int64_t ld, void* stream) {
  return guard(ctx, [&] {
    if (!rt || !rt->s) throw Error(RVCX_E_INVALID, "rt_model_rows: null stream group");
    RVCX_HIP(hipSetDevice(ctx->device));  // not a compute call: the pool the rows lie in is left as the hop left it
    rt_model_rows(*rt->s, gated, d_dst, ld, static_cast<hipStream_t>(stream));
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
    if (!ctx->ready[0] || !ctx->ready[1] || !ctx->ready[2]) throw Error(RVCX_E_STATE, "models not finalized");
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
  return guard(ctx, [&] {
    if (!ctx->ready[0] || !ctx->ready[1] || !ctx->ready[2]) throw Error(RVCX_E_STATE, "models not finalized");
    if (!d_audio || !n || !opts || !sids || !d_out || !n_out || B < 1)
      throw Error(RVCX_E_INVALID, "rvcx_pipeline_batch_v: bad arguments");
    set_device(ctx);
    pipeline_forward_rows(*ctx, d_audio, n, lda, B, *opts, sids, d_eps_z, d_eps_src, seed, d_out, ldo, n_out, d_f0, ldf,
                          nullptr, static_cast<hipStream_t>(stream));
  });
}
