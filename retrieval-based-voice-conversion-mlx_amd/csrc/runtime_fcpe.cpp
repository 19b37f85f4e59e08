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
//   ragged   fcpe_forward_v runs B utterances of different lengths through the same launches: activations
//            [B][F_max][C], a device array of the rows' frame counts F_b in every kernel that pads or reduces over time
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

// FCPE.forward (:657-665) on mel [B][F][n_mels] -> salience [B][F][out_dims]. dF (device, optional): stream b has
// dF[b] <= F frames in its F-row slot and mel rows from dF[b] on are zero. The k = 3 convs then see the zero padding
// of a run on that stream alone: stack.0 reads the zeroed mel rows, stack.3 the rows groupnorm_lrelu zeroes. The
// attention, the GroupNorm statistics and the depthwise conv end at dF[b]. Rows past dF[b] of the other activations
// hold whatever the row-wise ops make of them and never reach a valid row.
static void fcpe_net(Ctx& c, const float* mel, int F, int B, const int* dF, float* sal, hipStream_t s) {
  const FcpeCfg& g = c.fcfg;
  const int C = g.n_chans, inner = g.n_heads * g.dim_head;
  const int R = B * F;  // rows of every row-wise op (the callers check the range)
  // ---- input stack (:624-631): the k = 3 convs (zero pad 1) over each stream's own F rows
  float* x = c.buf<float>("fc.x", (size_t)R * C, s);
  float* x1 = c.buf<float>("fc.x1", (size_t)R * C, s);
  float* ln = c.buf<float>("fc.ln", (size_t)R * C, s);
  launch_conv(c, conv1d(mel, g.n_mels, F, g.n_mels, c.W("fc.stack0.w"), C, 3, 1, 1, c.W("fc.stack0.b"), x1, C, F, B),
              false, s);
  double* gnws = c.buf<double>("fc.gnws", (size_t)B * 4 * FCPE_GN_CHUNKS * 2, s);
  check(groupnorm_lrelu(x1, F, C, 4, c.W("fc.gn.g"), c.W("fc.gn.b"), 1e-5f, 0.01f, gnws, s, B, dF), "fcpe_groupnorm");
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
                              (long long)F * 3 * inner, (long long)F * inner, dF),
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
                           B, dF),
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
  ConvArgs a = lin(ln, C, R, C, c.W("fc.dense.w"), g.out_dims, c.W("fc.dense.b"), sal, g.out_dims);
  a.act = ACT_SIGMOID;
  launch_conv(c, a, false, s);
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
  const int F = (int)fcpe_frames(c, n);
  if (F > cap) throw Error(RVCX_E_CAPACITY, "fcpe: output needs " + std::to_string(F) + " frames per stream");
  float* mel = c.buf<float>("fc.mel", (size_t)B * F * g.n_mels, s);
  fcpe_mel(c, audio, n, ld, B, mel, s);
  float* sal = sal_out ? sal_out : c.buf<float>("fc.sal", (size_t)B * F * g.out_dims, s);
  fcpe_net(c, mel, F, B, nullptr, sal, s);
  // the decoders are row-wise: B F rows, f0 [B][F]
  check(fcpe_decode(sal, B * F, g.out_dims, c.W("fc.cent"), thr, mode, f0, s), "fcpe_decode");
  return F;
}

// FCPEInfer.__call__ on B utterances of nv[b] samples (host array; row b at audio + b ld) in one launch set: row b has
// F_b = fcpe_frames(nv[b]) frames inside [B][F_max][C]. Its f0 [F_b] lands at f0 + b ldf, its salience (optional) at
// sal_out + b ld_sal out_dims; nothing is written past F_b. Per row:
//   - the mel reflect-pads the row at its own end (samples past nv[b] are never read); its STFT frames past the row's
//     own are computed on the zeros after it and overwritten: row F_b - 1 = a copy of row F_b - 2, rows from F_b on zero;
//   - the network takes the rows' frame counts (fcpe_net); LayerNorm and every linear run once over the B F_max rows;
//   - the decode stops at F_b.
// Equal lengths are fcpe_forward_b, bit for bit, unless `sizing` (rvcx_workspace_bytes sizes the ragged form). A row of
// the mel's zero-padding branch among rows of different lengths is refused: mel_forward's per-row form reflects.
int64_t fcpe_forward_v(Ctx& c, const float* audio, const int64_t* nv, int64_t ld, int B, float thr, int mode, double* f0,
                       int64_t ldf, float* sal_out, int64_t ld_sal, hipStream_t s, bool sizing) {
  if (!c.ready[M]) throw Error(RVCX_E_STATE, "fcpe weights not finalized");
  if (mode < 0 || mode > 1) throw Error(RVCX_E_INVALID, "fcpe: decoder_mode must be 0 (local_argmax) or 1 (argmax)");
  if (B < 1 || B > 4096) throw Error(RVCX_E_INVALID, "fcpe: bad batch");
  const FcpeCfg& g = c.fcfg;
  int64_t n_max = 0, n_min = INT64_MAX;
  for (int b = 0; b < B; ++b) {
    if (nv[b] < 1 || nv[b] > INT32_MAX / 2) throw Error(RVCX_E_SHAPE, "fcpe: input length out of range");
    n_max = std::max(n_max, nv[b]);
    n_min = std::min(n_min, nv[b]);
  }
  const bool equal = n_min == n_max;
  if (ld < n_max && B > 1) throw Error(RVCX_E_INVALID, "fcpe: row stride shorter than the longest row");
  const int64_t pl = (g.win - g.hop) / 2, pr = (g.win - g.hop + 1) / 2;
  const bool ragged = B > 1 && (!equal || sizing);
  // the zero-padding branch (pr >= n in fcpe_mel) is a whole-batch form only
  if (ragged && std::max<int64_t>(pr, g.win - n_min - pl) >= n_min)
    throw Error(RVCX_E_SHAPE, "fcpe: a row of " + std::to_string(n_min) +
                                  " samples takes the mel's zero padding, which rows of different lengths do not run");
  const int64_t F_max = fcpe_frames(c, n_max);
  if (F_max > ldf) throw Error(RVCX_E_CAPACITY, "fcpe: output needs " + std::to_string(F_max) + " frames per row");
  if (sal_out && F_max > ld_sal)
    throw Error(RVCX_E_CAPACITY, "fcpe: salience needs " + std::to_string(F_max) + " frames per row");
  if (!ragged) {
    const int64_t F = F_max;
    const bool f0_tight = ldf == F || B == 1, sal_tight = !sal_out || ld_sal == F || B == 1;
    double* f0b = f0_tight ? f0 : c.buf<double>("fc.f0v", (size_t)B * F, s);
    float* sb = sal_tight ? sal_out : c.buf<float>("fc.salv", (size_t)B * F * g.out_dims, s);
    if (B == 1) {
      fcpe_forward(c, audio, n_max, thr, mode, 0, 0, f0b, sb, F, s);
    } else {
      fcpe_forward_b(c, audio, n_max, ld, B, thr, mode, f0b, F, sb, s);
    }
    if (!f0_tight)
      RVCX_HIP(hipMemcpy2DAsync(f0, (size_t)ldf * sizeof(double), f0b, (size_t)F * sizeof(double),
                                (size_t)F * sizeof(double), B, hipMemcpyDeviceToDevice, s));
    if (!sal_tight)
      RVCX_HIP(hipMemcpy2DAsync(sal_out, (size_t)ld_sal * g.out_dims * sizeof(float), sb,
                                (size_t)F * g.out_dims * sizeof(float), (size_t)F * g.out_dims * sizeof(float), B,
                                hipMemcpyDeviceToDevice, s));
    return F;
  }
  const MelSpec ms = mel_spec(g);
  if ((int64_t)B * F_max > INT32_MAX / std::max(4 * g.n_chans, 2 * ms.nbin()))
    throw Error(RVCX_E_SHAPE, "fcpe: too many frames");
  const int F = (int)F_max;
  // the reflect branch: the STFT gives n / hop frames, one fewer than F_b, for every row
  const int Fs = (int)((n_max + pl + pr - g.win) / g.hop + 1);
  if (Fs != F - 1) throw Error(RVCX_E_SHAPE, "fcpe: unexpected framing");
  // per-row lengths on device: n | F
  std::vector<int32_t> hl(2 * (size_t)B);
  int F_min = F;
  for (int b = 0; b < B; ++b) {
    hl[b] = (int32_t)nv[b];
    hl[B + b] = (int32_t)fcpe_frames(c, nv[b]);
    F_min = std::min(F_min, hl[B + b]);
  }
  int32_t* dl = c.buf<int32_t>("fc.lens", hl.size(), s);
  RVCX_HIP(hipMemcpyAsync(dl, hl.data(), sizeof(int32_t) * hl.size(), hipMemcpyHostToDevice, s));
  const int32_t *dn = dl, *dF = dl + B;
  float* mel = c.buf<float>("fc.mel", (size_t)B * F * g.n_mels, s);
  mel_forward(c, ms, "fc.", audio, n_max, ld, B, MelFrames{pl, pr, false, Fs, F, true}, mel, s, dn);
  check(fcpe_mel_tail_v(mel, B, dF, F, F_min, g.n_mels, s), "fcpe_mel_tail");
  float* sal = c.buf<float>("fc.sal", (size_t)B * F * g.out_dims, s);
  fcpe_net(c, mel, F, B, dF, sal, s);
  if (sal_out)
    for (int b = 0; b < B; ++b)
      RVCX_HIP(hipMemcpyAsync(sal_out + (size_t)b * ld_sal * g.out_dims, sal + (size_t)b * F * g.out_dims,
                              (size_t)hl[B + b] * g.out_dims * sizeof(float), hipMemcpyDeviceToDevice, s));
  check(fcpe_decode_v(sal, B, dF, F, g.out_dims, c.W("fc.cent"), thr, mode, f0, ldf, s), "fcpe_decode");
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
