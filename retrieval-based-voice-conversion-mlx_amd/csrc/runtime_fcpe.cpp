// FCPE pitch estimator on device (f0 method "fcpe" of rvc/): rvc/lib/predictors/FCPE.py -- Wav2Mel / STFT.get_mel
// (:102-168, :790-813), FCPE.forward (:649-681: conv stack, PCmer = n_layers x (Performer self-attention + Conformer
// conv module), LayerNorm, weight-normed dense_out, sigmoid), the cents decoders (:683-714) and
// FCPEF0Predictor.post_process (:877-902). Time-major [frame][channel] throughout:
//   mel      the STFT as a conv over 32-sample rows (win / 32 taps, stride hop / 32: the RMVPE front end's form, with
//            this model's window, hop and padding), sqrt(re^2 + im^2 + 1e-9), the Slaney mel basis, log(clamp(1e-5))
//   convs    stack.0 / stack.3 (k 3) and every Linear / 1x1 conv on the implicit-GEMM family (launch_conv)
//   attn     to_q | to_k | to_v as one GEMM into [F][3 x 512], then performer_attn.hip on the 8 heads in place
//   conformer LN -> 1x1 (C -> 4C) -> GLU + depthwise k 31 + Swish (one kernel, fcpe.hip) -> 1x1 (2C -> C)
//   batch    fcpe_forward_b runs B streams of one length in one set of launches per layer (a realtime hop's f0 with
//            rvcx_rt_desc::f0_method 1, rvcx_fcpe_b): activations [B][F][C], row-wise ops on the B F rows, everything
//            padded or reduced over time per stream. fcpe_forward is its B = 1 case plus the interp_uv / pad_to tail
#include <cmath>

#include "model_build.h"

namespace rvcx {

namespace {
constexpr int M = RVCX_MODEL_FCPE;  // model slot

// STFT.get_mel (FCPE.py:123-126, :154): librosa's default (Slaney) basis, sqrt(re^2 + im^2 + 1e-9); n_fft == win
MelSpec mel_spec(const FcpeCfg& g) { return {g.sr, g.win, g.hop, g.n_mels, g.fmin, g.fmax, false, 1e-9f}; }

std::string lp(int i) { return "decoder._layers." + std::to_string(i) + "."; }
std::string dn(int i, const char* what) { return "fc.l" + std::to_string(i) + "." + what; }

}  // namespace

// Validates the FCPE module's state dict against the configured sizes and packs it: conv weights to [tap][O][I],
// to_q | to_k | to_v stacked to one [3 x 512][C] weight, the depthwise kernel to [k][2C].
void finalize_fcpe(Ctx& c) {
  FcpeCfg& g = c.fcfg;
  if (g.n_fft != g.win) throw Error(RVCX_E_SHAPE, "fcpe: n_fft != win_size is not supported");
  if (g.win < 32 || g.win % 32 || g.hop < 32 || g.hop % 32 || g.hop > g.win)
    throw Error(RVCX_E_SHAPE, "fcpe: win_size and hop_size must be multiples of 32 with hop_size <= win_size");
  if (g.n_mels < 32 || g.n_mels % 32) throw Error(RVCX_E_SHAPE, "fcpe: num_mels must be a multiple of 32");
  if (g.n_chans < 32 || g.n_chans % 32 || g.n_chans > 1024)
    throw Error(RVCX_E_SHAPE, "fcpe: n_chans must be a multiple of 32, at most 1024");
  if (g.n_layers < 1 || g.out_dims < 9 || g.sr < 1 || !(g.fmax > g.fmin) || g.fmin < 0)
    throw Error(RVCX_E_INVALID, "fcpe: bad configuration");
  const int C = g.n_chans, inner = g.n_heads * g.dim_head, K = g.conv_k;
  auto pm = c.host[M].find(lp(0) + "attn.fast_attention.projection_matrix");
  if (pm == c.host[M].end() || pm->second.shape.size() != 2)
    throw Error(RVCX_E_STATE, "missing weight: " + lp(0) + "attn.fast_attention.projection_matrix");
  g.n_feat = (int)pm->second.shape[0];
  if (g.n_feat < 1 || g.n_feat > PERFORMER_MAX_FEATURES)
    throw Error(RVCX_E_SHAPE, "fcpe: projection_matrix rows (nb_features) must be in [1, 512]");
  c.alloc_weight("fc.stft", stft_weights(g.win));
  c.alloc_weight("fc.mel", mel_basis(mel_spec(g)));
  c.alloc_weight("fc.stack0.w", pack_conv1d(host_weight(c, M, "stack.0.weight", {C, g.n_mels, 3})));
  c.alloc_weight("fc.stack0.b", host_weight(c, M, "stack.0.bias", {C}).v);
  c.alloc_weight("fc.gn.g", host_weight(c, M, "stack.1.weight", {C}).v);
  c.alloc_weight("fc.gn.b", host_weight(c, M, "stack.1.bias", {C}).v);
  c.alloc_weight("fc.stack3.w", pack_conv1d(host_weight(c, M, "stack.3.weight", {C, C, 3})));
  c.alloc_weight("fc.stack3.b", host_weight(c, M, "stack.3.bias", {C}).v);
  for (int i = 0; i < g.n_layers; ++i) {
    const std::string p = lp(i);
    c.alloc_weight(dn(i, "ln.g"), host_weight(c, M, p + "norm.weight", {C}).v);
    c.alloc_weight(dn(i, "ln.b"), host_weight(c, M, p + "norm.bias", {C}).v);
    std::vector<float> w, b;
    for (const char* n : {"to_q", "to_k", "to_v"}) {
      const auto& wv = host_weight(c, M, p + "attn." + n + ".weight", {inner, C}).v;
      const auto& bv = host_weight(c, M, p + "attn." + n + ".bias", {inner}).v;
      w.insert(w.end(), wv.begin(), wv.end());
      b.insert(b.end(), bv.begin(), bv.end());
    }
    c.alloc_weight(dn(i, "qkv.w"), w);
    c.alloc_weight(dn(i, "qkv.b"), b);
    c.alloc_weight(dn(i, "proj"),
                   host_weight(c, M, p + "attn.fast_attention.projection_matrix", {g.n_feat, g.dim_head}).v);
    c.alloc_weight(dn(i, "out.w"), host_weight(c, M, p + "attn.to_out.weight", {C, inner}).v);
    c.alloc_weight(dn(i, "out.b"), host_weight(c, M, p + "attn.to_out.bias", {C}).v);
    c.alloc_weight(dn(i, "cf.ln.g"), host_weight(c, M, p + "conformer.net.0.weight", {C}).v);
    c.alloc_weight(dn(i, "cf.ln.b"), host_weight(c, M, p + "conformer.net.0.bias", {C}).v);
    c.alloc_weight(dn(i, "cf.pw1.w"), host_weight(c, M, p + "conformer.net.2.weight", {4 * C, C, 1}).v);
    c.alloc_weight(dn(i, "cf.pw1.b"), host_weight(c, M, p + "conformer.net.2.bias", {4 * C}).v);
    const auto& dw = host_weight(c, M, p + "conformer.net.4.conv.weight", {2 * C, 1, K}).v;
    std::vector<float> dwt((size_t)K * 2 * C);
    for (int ch = 0; ch < 2 * C; ++ch)
      for (int k = 0; k < K; ++k) dwt[(size_t)k * 2 * C + ch] = dw[(size_t)ch * K + k];
    c.alloc_weight(dn(i, "cf.dw.w"), dwt);
    c.alloc_weight(dn(i, "cf.dw.b"), host_weight(c, M, p + "conformer.net.4.conv.bias", {2 * C}).v);
    c.alloc_weight(dn(i, "cf.pw2.w"), host_weight(c, M, p + "conformer.net.6.weight", {C, 2 * C, 1}).v);
    c.alloc_weight(dn(i, "cf.pw2.b"), host_weight(c, M, p + "conformer.net.6.bias", {C}).v);
  }
  c.alloc_weight("fc.norm.g", host_weight(c, M, "norm.weight", {C}).v);
  c.alloc_weight("fc.norm.b", host_weight(c, M, "norm.bias", {C}).v);
  c.alloc_weight("fc.dense.w", host_weight(c, M, "dense_out.weight", {g.out_dims, C}).v);
  c.alloc_weight("fc.dense.b", host_weight(c, M, "dense_out.bias", {g.out_dims}).v);
  c.alloc_weight("fc.cent", host_weight(c, M, "cent_table", {g.out_dims}).v);
}

// the frames FCPEInfer gives for n samples: n / hop + 1, or one more than the STFT's when that is fewer
// (Wav2Mel.extract_mel appends one copy of the last frame, FCPE.py:808-812)
int64_t fcpe_frames(const Ctx& c, int64_t n) {
  const FcpeCfg& g = c.fcfg;
  const int64_t pl = (g.win - g.hop) / 2, pr = std::max<int64_t>((g.win - g.hop + 1) / 2, g.win - n - pl);
  const int64_t fs = (n + pl + pr - g.win) / g.hop + 1, nf = n / g.hop + 1;
  return nf > fs ? fs + 1 : nf;
}

int64_t fcpe_decode_run(Ctx& c, const float* sal, int64_t F, float thr, int mode, int interp_uv, int64_t pad_to,
                        double* f0, hipStream_t s) {
  if (!c.ready[M]) throw Error(RVCX_E_STATE, "fcpe weights not finalized");
  if (mode < 0 || mode > 1) throw Error(RVCX_E_INVALID, "fcpe: decoder_mode must be 0 (local_argmax) or 1 (argmax)");
  const FcpeCfg& g = c.fcfg;
  if (F < 1 || F > INT32_MAX / g.out_dims || pad_to > INT32_MAX / 2) throw Error(RVCX_E_SHAPE, "fcpe: too many frames");
  if (!interp_uv) {
    check(fcpe_decode(sal, (int)F, g.out_dims, c.W("fc.cent"), thr, mode, f0, s), "fcpe_decode");
    return F;
  }
  const int64_t n = pad_to > 0 ? pad_to : F;
  double* raw = c.buf<double>("fc.f0raw", (size_t)F, s);
  int* links = c.buf<int>("fc.links", (size_t)2 * n, s);
  check(fcpe_decode(sal, (int)F, g.out_dims, c.W("fc.cent"), thr, mode, raw, s), "fcpe_decode");
  check(fcpe_post_process(raw, (int)F, (int)n, g.hop, g.sr, links, f0, s), "fcpe_post_process");
  return n;
}

// Wav2Mel.extract_mel (FCPE.py:790-813; STFT.get_mel :133-168) on B streams of n samples (row b at audio + b ld): the
// log-mel [B][F][n_mels] into `mel` (F = fcpe_frames(n) rows per stream). Every stream is padded, framed and, when the
// STFT gives one frame fewer than F, extended by a copy of its own last frame: the STFT conv runs in launch_conv's
// batch form over the streams' own padded rows, so no frame reads across a stream boundary. Returns F.
int fcpe_mel(Ctx& c, const float* audio, int64_t n, int64_t ld, int B, float* mel, hipStream_t s) {
  if (!c.ready[M]) throw Error(RVCX_E_STATE, "fcpe weights not finalized");
  const FcpeCfg& g = c.fcfg;
  if (n < 1 || n > INT32_MAX / 2) throw Error(RVCX_E_SHAPE, "fcpe: input length out of range");
  if (B < 1 || B > 4096 || ld < n) throw Error(RVCX_E_INVALID, "fcpe: bad batch");
  const MelSpec ms = mel_spec(g);
  const int64_t pl = (g.win - g.hop) / 2, pr = std::max<int64_t>((g.win - g.hop + 1) / 2, g.win - n - pl);
  const int Fs = (int)((n + pl + pr - g.win) / g.hop + 1);
  const int F = (int)fcpe_frames(c, n), Fm = std::min(Fs, F);
  if ((int64_t)B * F > INT32_MAX / std::max(4 * g.n_chans, 2 * ms.nbin()))
    throw Error(RVCX_E_SHAPE, "fcpe: too many frames");
  // torch pads with zeros when the reflection would not fit (:138)
  mel_forward(c, ms, "fc.", audio, n, ld, B, MelFrames{pl, pr, pr >= n, Fm, F, true}, mel, s);
  if (F > Fm) check(fcpe_dup_last_frame(mel, B, F, g.n_mels, s), "fcpe_dup_last_frame");
  return F;
}

// FCPEInfer.__call__ on B streams of n samples (row b at audio + b ld): f0 [B][F] (the raw track: zeros where
// unvoiced), salience [B][F][out_dims] optional. Activations are [B][F][C] with the streams back to back, so
// LayerNorm and every linear run once on the B F rows; what the network reduces or pads over time -- the mel's
// framing, the k = 3 convs' zero padding (launch_conv's batch form), the GroupNorm statistics, the Performer's ctx /
// ksum / row maximum / denominator, the depthwise conv's zero padding -- is per stream. B = 1 is fcpe_forward.
int64_t fcpe_forward_b(Ctx& c, const float* audio, int64_t n, int64_t ld, int B, float thr, int mode, double* f0,
                       int64_t cap, float* sal_out, hipStream_t s) {
  if (!c.ready[M]) throw Error(RVCX_E_STATE, "fcpe weights not finalized");
  if (mode < 0 || mode > 1) throw Error(RVCX_E_INVALID, "fcpe: decoder_mode must be 0 (local_argmax) or 1 (argmax)");
  const FcpeCfg& g = c.fcfg;
  if (n < 1 || n > INT32_MAX / 2) throw Error(RVCX_E_SHAPE, "fcpe: input length out of range");
  if (B < 1 || B > 4096 || ld < n) throw Error(RVCX_E_INVALID, "fcpe: bad batch");
  const int C = g.n_chans, inner = g.n_heads * g.dim_head;
  const int F = (int)fcpe_frames(c, n);
  if (F > cap) throw Error(RVCX_E_CAPACITY, "fcpe: output needs " + std::to_string(F) + " frames per stream");
  const int R = B * F;  // rows of every row-wise op (fcpe_mel checks the range)
  float* mel = c.buf<float>("fc.mel", (size_t)R * g.n_mels, s);
  fcpe_mel(c, audio, n, ld, B, mel, s);
  // ---- input stack (:624-631): the k = 3 convs (zero pad 1) over each stream's own F rows
  float* x = c.buf<float>("fc.x", (size_t)R * C, s);
  float* x1 = c.buf<float>("fc.x1", (size_t)R * C, s);
  float* ln = c.buf<float>("fc.ln", (size_t)R * C, s);
  launch_conv(c, conv1d(mel, g.n_mels, F, g.n_mels, c.W("fc.stack0.w"), C, 3, 1, 1, c.W("fc.stack0.b"), x1, C, F, B),
              false, s);
  double* gnws = c.buf<double>("fc.gnws", (size_t)B * 4 * FCPE_GN_CHUNKS * 2, s);
  check(groupnorm_lrelu(x1, F, C, 4, c.W("fc.gn.g"), c.W("fc.gn.b"), 1e-5f, 0.01f, gnws, s, B), "fcpe_groupnorm");
  launch_conv(c, conv1d(x1, C, F, C, c.W("fc.stack3.w"), C, 3, 1, 1, c.W("fc.stack3.b"), x, C, F, B), false, s);
  // ---- PCmer (:270-283)
  float* qkv = c.buf<float>("fc.qkv", (size_t)R * 3 * inner, s);
  float* att = c.buf<float>("fc.att", (size_t)R * inner, s);
  float* h4 = c.buf<float>("fc.h4", (size_t)R * 4 * C, s);
  float* dw = c.buf<float>("fc.dw", (size_t)R * 2 * C, s);
  float* aws = c.buf<float>("fc.attws", (size_t)performer_ws_floats(g.n_heads, F, g.n_feat, B), s);
  for (int i = 0; i < g.n_layers; ++i) {
    // x1 = x + to_out(attention(to_q, to_k, to_v of LN(x)))
    check(layernorm_rows(x, nullptr, ln, c.W(dn(i, "ln.g")), c.W(dn(i, "ln.b")), R, C, 1e-5f, nullptr, s), "fcpe_ln");
    launch_conv(c, lin(ln, C, R, C, c.W(dn(i, "qkv.w")), 3 * inner, c.W(dn(i, "qkv.b")), qkv, 3 * inner), false, s);
    check(performer_attention(qkv, qkv + inner, qkv + 2 * inner, g.dim_head, 3 * inner, g.n_heads, F,
                              c.W(dn(i, "proj")), g.n_feat, aws, att, g.dim_head, inner, s, B,
                              (long long)F * 3 * inner, (long long)F * inner),
          "performer_attention");
    {
      ConvArgs a = lin(att, inner, R, inner, c.W(dn(i, "out.w")), C, c.W(dn(i, "out.b")), x1, C);
      a.res = x;
      a.ldr = C;
      a.res_mode = RES_ADD_POST;
      launch_conv(c, a, false, s);
    }
    // x = x1 + conformer(x1)
    check(layernorm_rows(x1, nullptr, ln, c.W(dn(i, "cf.ln.g")), c.W(dn(i, "cf.ln.b")), R, C, 1e-5f, nullptr, s),
          "fcpe_ln");
    launch_conv(c, lin(ln, C, R, C, c.W(dn(i, "cf.pw1.w")), 4 * C, c.W(dn(i, "cf.pw1.b")), h4, 4 * C), false, s);
    check(glu_dwconv_swish(h4, F, 2 * C, c.W(dn(i, "cf.dw.w")), c.W(dn(i, "cf.dw.b")), g.conv_k, g.conv_k / 2, dw, s,
                           B),
          "fcpe_dwconv");
    {
      ConvArgs a = lin(dw, 2 * C, R, 2 * C, c.W(dn(i, "cf.pw2.w")), C, c.W(dn(i, "cf.pw2.b")), x, C);
      a.res = x1;
      a.ldr = C;
      a.res_mode = RES_ADD_POST;
      launch_conv(c, a, false, s);
    }
  }
  // ---- head (:663-665)
  check(layernorm_rows(x, nullptr, ln, c.W("fc.norm.g"), c.W("fc.norm.b"), R, C, 1e-5f, nullptr, s), "fcpe_ln");
  float* sal = sal_out ? sal_out : c.buf<float>("fc.sal", (size_t)R * g.out_dims, s);
  {
    ConvArgs a = lin(ln, C, R, C, c.W("fc.dense.w"), g.out_dims, c.W("fc.dense.b"), sal, g.out_dims);
    a.act = ACT_SIGMOID;
    launch_conv(c, a, false, s);
  }
  // the decoders are row-wise: B F rows, f0 [B][F]
  check(fcpe_decode(sal, R, g.out_dims, c.W("fc.cent"), thr, mode, f0, s), "fcpe_decode");
  return F;
}

// One utterance: the B = 1 case of fcpe_forward_b, then FCPEF0Predictor.post_process when interp_uv.
int64_t fcpe_forward(Ctx& c, const float* audio, int64_t n, float thr, int mode, int interp_uv, int64_t pad_to,
                     double* f0, float* sal_out, int64_t cap, hipStream_t s) {
  if (!c.ready[M]) throw Error(RVCX_E_STATE, "fcpe weights not finalized");
  const FcpeCfg& g = c.fcfg;
  if (n < 1 || n > INT32_MAX / 2) throw Error(RVCX_E_SHAPE, "fcpe: input length out of range");
  const int64_t F = fcpe_frames(c, n);
  const int64_t n_out = interp_uv && pad_to > 0 ? pad_to : F;
  if (n_out > cap) throw Error(RVCX_E_CAPACITY, "fcpe: output needs " + std::to_string(n_out) + " frames");
  if (!interp_uv) return fcpe_forward_b(c, audio, n, n, 1, thr, mode, f0, cap, sal_out, s);
  if (n_out > INT32_MAX / 2) throw Error(RVCX_E_SHAPE, "fcpe: too many frames");
  double* raw = c.buf<double>("fc.f0raw", (size_t)F, s);
  int* links = c.buf<int>("fc.links", (size_t)2 * n_out, s);
  fcpe_forward_b(c, audio, n, n, 1, thr, mode, raw, F, sal_out, s);
  check(fcpe_post_process(raw, (int)F, (int)n_out, g.hop, g.sr, links, f0, s), "fcpe_post_process");
  return n_out;
}

}  // namespace rvcx
