// FCPE pitch estimator on device (f0 method "fcpe" of rvc/): rvc/lib/predictors/FCPE.py -- Wav2Mel / STFT.get_mel
// (:102-168, :790-813), FCPE.forward (:649-681: conv stack, PCmer = n_layers x (Performer self-attention + Conformer
// conv module), LayerNorm, weight-normed dense_out, sigmoid), the cents decoders (:683-714) and
// FCPEF0Predictor.post_process (:877-902). Time-major [frame][channel] throughout:
//   mel      the STFT as a conv over 32-sample rows (win / 32 taps, stride hop / 32: the RMVPE front end's form, with
//            this model's window, hop and padding), sqrt(re^2 + im^2 + 1e-9), the Slaney mel basis, log(clamp(1e-5))
//   convs    stack.0 / stack.3 (k 3) and every Linear / 1x1 conv on the implicit-GEMM family (launch_conv)
//   attn     to_q | to_k | to_v as one GEMM into [F][3 x 512], then performer_attn.hip on the 8 heads in place
//   conformer LN -> 1x1 (C -> 4C) -> GLU + depthwise k 31 + Swish (one kernel, fcpe.hip) -> 1x1 (2C -> C)
//   rows     fcpe_rows is the one pass over B rows, of one length (fcpe_forward_b: a realtime hop's f0 with
//            rvcx_rt_desc::f0_method 1; fcpe_forward is B = 1 plus the interp_uv / pad_to tail) or of their own lengths
//            (fcpe_forward_v): a device array of the frame counts F_b in every kernel that pads or reduces over time
#include <cmath>

#include "model_build.h"
#include "rows.h"

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

// How Wav2Mel.extract_mel frames n samples (FCPE.py:805-813; STFT.get_mel :133-168): pl / pr samples of padding (zeros
// when the reflection would not fit), Fs STFT frames and F in all: n / hop + 1, or Fs + 1 when that is fewer (:808-812)
struct Framing {
  int64_t pl, pr, Fs, F;
  bool zero_pad;
};
static Framing framing(const FcpeCfg& g, int64_t n) {
  const int64_t pl = (g.win - g.hop) / 2, pr = std::max<int64_t>((g.win - g.hop + 1) / 2, g.win - n - pl);
  const int64_t Fs = (n + pl + pr - g.win) / g.hop + 1, nf = n / g.hop + 1;
  return {pl, pr, Fs, nf > Fs ? Fs + 1 : nf, pr >= n};
}

// what every entry checks: the model, the decoder mode and the rows (nv == nullptr: B of n samples; none by default)
static Rows checked_rows(const Ctx& c, int m, const int64_t* nv = nullptr, int64_t n = 1, int B = 1, int64_t ld = 0) {
  if (!c.ready[M]) throw Error(RVCX_E_STATE, "fcpe weights not finalized");
  if (m < 0 || m > 1) throw Error(RVCX_E_INVALID, "fcpe: decoder_mode must be 0 (local_argmax) or 1 (argmax)");
  if (B > 4096) throw Error(RVCX_E_INVALID, "fcpe: bad batch");
  const Rows r = nv ? Rows("fcpe", nv, B, ld) : Rows("fcpe", n, B, ld);
  if (r.n_min < 1 || r.n_max > INT32_MAX / 2) throw Error(RVCX_E_SHAPE, "fcpe: input length out of range");
  return r;
}

// The mel stage: B streams, the longest of n samples and framed as `fr`, -> the log-mel [B][F][n_mels], each stream
// padded and framed on its own, with a copy of its last frame when the STFT gives one fewer than F. dn / dF (device):
// stream b has dn[b] samples and dF[b] >= F_min frames; row F_b - 1 = row F_b - 2, zeros from F_b on.
static void mel_stage(Ctx& c, const float* audio, int64_t n, int64_t ld, int B, const Framing& fr, const int32_t* dn,
               const int32_t* dF, int F_min, float* mel, hipStream_t s) {
  const FcpeCfg& g = c.fcfg;
  const MelSpec ms = mel_spec(g);
  if ((int64_t)B * fr.F > INT32_MAX / std::max(4 * g.n_chans, 2 * ms.nbin()))
    throw Error(RVCX_E_SHAPE, "fcpe: too many frames");
  const int F = (int)fr.F, Fm = (int)std::min(fr.Fs, fr.F);
  mel_forward(c, ms, "fc.", audio, n, ld, B, MelFrames{fr.pl, fr.pr, fr.zero_pad, Fm, F, true}, mel, s, dn);
  if (dF) check(fcpe_mel_tail_v(mel, B, dF, F, F_min, g.n_mels, s), "fcpe_mel_tail");
  else if (F > Fm) check(fcpe_dup_last_frame(mel, B, F, g.n_mels, s), "fcpe_dup_last_frame");
}

// FCPEF0Predictor.post_process of the raw track [F] (or nothing, when it was written to f0 itself) -> f0 [n]
static void post_process(Ctx& c, const double* raw, int64_t F, int64_t n, double* f0, hipStream_t s) {
  if (raw == f0) return;
  int* links = c.buf<int>("fc.links", (size_t)2 * n, s);
  check(fcpe_post_process(raw, (int)F, (int)n, c.fcfg.hop, c.fcfg.sr, links, f0, s), "fcpe_post_process");
}

int64_t fcpe_frames(const Ctx& c, int64_t n) { return framing(c.fcfg, n).F; }

int64_t fcpe_decode_run(Ctx& c, const float* sal, int64_t F, float thr, int mode, int interp_uv, int64_t pad_to,
                        double* f0, hipStream_t s) {
  checked_rows(c, mode);
  const int nb = c.fcfg.out_dims;
  if (F < 1 || F > INT32_MAX / nb || pad_to > INT32_MAX / 2) throw Error(RVCX_E_SHAPE, "fcpe: too many frames");
  const int64_t n = interp_uv && pad_to > 0 ? pad_to : F;
  double* raw = interp_uv ? c.buf<double>("fc.f0raw", (size_t)F, s) : f0;
  check(fcpe_decode(sal, (int)F, nb, c.W("fc.cent"), thr, mode, raw, s), "fcpe_decode");
  post_process(c, raw, F, n, f0, s);
  return n;
}

int fcpe_mel(Ctx& c, const float* audio, int64_t n, int64_t ld, int B, float* mel, hipStream_t s) {
  checked_rows(c, 0, nullptr, n, B, ld);
  const Framing fr = framing(c.fcfg, n);
  mel_stage(c, audio, n, ld, B, fr, nullptr, nullptr, 0, mel, s);
  return (int)fr.F;
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

// The one FCPE pass behind fcpe_forward, _b and _v (runtime.h), FCPEInfer.__call__: mel -> network -> decode on the B
// rows `r` describes (row b at audio + b ld). The raw track of row b lands at f0 + b ldf, its salience (optional) at
// sal_out + b ld_sal out_dims. Activations are [B][F][C] with the rows back to back, so LayerNorm and every linear run
// once on the B F rows; what the network reduces or pads over time -- the mel's framing, the k = 3 convs' zero padding
// (launch_conv's batch form), the GroupNorm statistics, the Performer's ctx / ksum / row maximum / denominator, the
// depthwise conv's zero padding -- is per row.
// nv == nullptr: B rows of r.n_max samples; the network writes the caller's salience (or its staging, below) in place.
// nv[B] (host): row b has nv[b] samples and F_b = fcpe_frames(nv[b]) frames inside [B][F_max][C]; nothing written past
// F_b. Per row:
//   - the mel reflect-pads the row at its own end (samples past nv[b] are never read) and ends it as mel_stage says;
//   - the network takes the rows' frame counts (fcpe_net); LayerNorm and every linear run once over the B F_max rows;
//   - the decode and the salience copy stop at F_b.
// A row of the zero-padding branch among rows of different lengths is refused: mel_forward's per-row form reflects.
static int64_t fcpe_rows(Ctx& c, const float* audio, const Rows& r, const int64_t* nv, int64_t ld, float thr, int mode,
                         double* f0, int64_t ldf, float* sal_out, int64_t ld_sal, hipStream_t s) {
  const FcpeCfg& g = c.fcfg;
  const int B = r.B, nb = g.out_dims;
  // the zero-padding branch is a whole-batch form only
  if (nv && framing(g, r.n_min).zero_pad)
    throw Error(RVCX_E_SHAPE, "fcpe: a row of " + std::to_string(r.n_min) +
                                  " samples takes the mel's zero padding, which rows of different lengths do not run");
  const Framing fr = framing(g, r.n_max);
  if (fr.F > ldf) throw Error(RVCX_E_CAPACITY, "fcpe: output needs " + std::to_string(fr.F) + " frames per row");
  if (sal_out && fr.F > ld_sal)
    throw Error(RVCX_E_CAPACITY, "fcpe: salience needs " + std::to_string(fr.F) + " frames per row");
  const int F = (int)fr.F;
  // the strides the pass itself writes: the caller's with lengths, else back to back and staged where those are wider
  const int64_t sf = nv ? ldf : F, ss = nv ? ld_sal : F;
  const Staged<double> f0s(c, "fc.f0v", f0, ldf, sf, B, s);
  const Staged<float> sals(c, "fc.salv", sal_out, ld_sal * nb, ss * nb, B, s);
  // the reflect branch: the STFT gives n / hop frames, one fewer than F_b, for every row
  if (nv && fr.Fs != F - 1) throw Error(RVCX_E_SHAPE, "fcpe: unexpected framing");
  // per-row lengths on device: n | F
  LenCols len(2, nv ? B : 0);
  const int32_t *dn = nullptr, *dF = nullptr;
  int F_min = F;
  if (nv) {
    for (int b = 0; b < B; ++b) {
      len.at(0, b) = (int32_t)nv[b];
      len.at(1, b) = (int32_t)framing(g, nv[b]).F;
      F_min = std::min(F_min, len.at(1, b));
    }
    len.upload(c, "fc.lens", s);
    dn = len.col(0), dF = len.col(1);
  }
  float* mel = c.buf<float>("fc.mel", (size_t)B * F * g.n_mels, s);
  mel_stage(c, audio, r.n_max, ld, B, fr, dn, dF, F_min, mel, s);
  float* sal = !nv && sal_out ? sals.p : c.buf<float>("fc.sal", (size_t)B * F * nb, s);
  fcpe_net(c, mel, F, B, dF, sal, s);
  if (nv) {
    if (sal_out)
      for (int b = 0; b < B; ++b)
        RVCX_HIP(hipMemcpyAsync(sal_out + (size_t)b * ld_sal * nb, sal + (size_t)b * F * nb,
                                (size_t)len.at(1, b) * nb * sizeof(float), hipMemcpyDeviceToDevice, s));
    check(fcpe_decode_v(sal, B, dF, F, nb, c.W("fc.cent"), thr, mode, f0, ldf, s), "fcpe_decode");
  } else {
    // the decoders are row-wise: B F rows, f0 [B][F]
    check(fcpe_decode(sal, B * F, nb, c.W("fc.cent"), thr, mode, f0s.p, s), "fcpe_decode");
  }
  f0s.copy_out(s);
  sals.copy_out(s);
  return F;
}

int64_t fcpe_forward_b(Ctx& c, const float* audio, int64_t n, int64_t ld, int B, float thr, int mode, double* f0,
                       int64_t cap, float* sal_out, hipStream_t s) {
  const Rows r = checked_rows(c, mode, nullptr, n, B, ld);
  const int64_t lf = std::min(cap, fcpe_frames(c, n));  // back to back; a cap below the frame count is refused
  return fcpe_rows(c, audio, r, nullptr, ld, thr, mode, f0, lf, sal_out, lf, s);
}

int64_t fcpe_forward_v(Ctx& c, const float* audio, const int64_t* nv, int64_t ld, int B, float thr, int mode, double* f0,
                       int64_t ldf, float* sal_out, int64_t ld_sal, hipStream_t s, bool sizing) {
  const Rows r = checked_rows(c, mode, nv, 0, B, ld);
  const bool ragged = B > 1 && (!r.equal || sizing);
  return fcpe_rows(c, audio, r, ragged ? nv : nullptr, ld, thr, mode, f0, ldf, sal_out, ld_sal, s);
}

int64_t fcpe_forward(Ctx& c, const float* audio, int64_t n, float thr, int mode, int interp_uv, int64_t pad_to,
                     double* f0, float* sal_out, int64_t cap, hipStream_t s) {
  const Rows r = checked_rows(c, mode, nullptr, n, 1, n);
  const int64_t F = fcpe_frames(c, n), n_out = interp_uv && pad_to > 0 ? pad_to : F;
  if (n_out > cap) throw Error(RVCX_E_CAPACITY, "fcpe: output needs " + std::to_string(n_out) + " frames");
  if (interp_uv && n_out > INT32_MAX / 2) throw Error(RVCX_E_SHAPE, "fcpe: too many frames");
  double* raw = interp_uv ? c.buf<double>("fc.f0raw", (size_t)F, s) : f0;
  fcpe_rows(c, audio, r, nullptr, n, thr, mode, raw, F, sal_out, F, s);
  post_process(c, raw, F, n_out, f0, s);
  return n_out;
}

}  // namespace rvcx
