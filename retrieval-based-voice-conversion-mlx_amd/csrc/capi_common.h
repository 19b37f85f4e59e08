// What the two extern "C" translation units share: capi.cpp (include/rvcx.h, the product ABI) and capi_test.cpp
// (include/rvcx_test.h, the kernel-level test entries). Every entry point converts C++ exceptions into an rvcx_status
// and stores the message for rvcx_last_error.
#pragma once
#include <exception>

#include "runtime.h"

struct rvcx_ctx : public rvcx::Ctx {};
struct rvcx_rt {
  rvcx::RtState* s = nullptr;
};

namespace rvcx {

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
inline void set_device(rvcx_ctx* c) {
  RVCX_HIP(hipSetDevice(c->device));
  c->check_device_status();
  c->begin_call();
}

// the synthesizer configuration a descriptor names (rvcx_set_synth_config, rvcx_dec_margin_frames)
inline SynthCfg synth_cfg_of(const rvcx_synth_desc* d) {
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

}  // namespace rvcx
