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

#include "runtime.h"

namespace rvcx {

namespace {
constexpr int M = RVCX_MODEL_FCPE;  // model slot

const HostTensor& getf(Ctx& c, const std::string& n, std::vector<int64_t> shape) {
  auto it = c.host[M].find(n);
  if (it == c.host[M].end()) throw Error(RVCX_E_STATE, "missing weight: " + n);
  if (it->second.shape != shape) {
    std::string got, want;
    for (auto s : it->second.shape) got += std::to_string(s) + ",";
    for (auto s : shape) want += std::to_string(s) + ",";
    throw Error(RVCX_E_SHAPE, "weight " + n + " has shape (" + got + ") expected (" + want + ")");
  }
  return it->second;
}

std::vector<float> pack_k(const HostTensor& t) {  // Conv1d [O][I][K] -> [K][O][I]
  const int64_t O = t.shape[0], I = t.shape[1], K = t.shape[2];
  std::vector<float> out(t.v.size());
  for (int64_t o = 0; o < O; ++o)
    for (int64_t i = 0; i < I; ++i)
      for (int64_t k = 0; k < K; ++k) out[(k * O + o) * I + i] = t.v[(o * I + i) * K + k];
  return out;
}

// y [rows][N] = x [rows][K] W^T + bias, W [N][K]
ConvArgs lin(const float* x, int ldx, int rows, int K, const float* w, int N, const float* bias, float* y, int ldy) {
  ConvArgs a;
  a.x = x;
  a.ldx = ldx;
  a.T_in = rows;
  a.C_in = K;
  a.w = w;
  a.ldw = K;
  a.taps = 1;
  a.y = y;
  a.ldy = ldy;
  a.T_out = rows;
  a.N = N;
  a.bias = bias;
  return a;
}

ConvArgs conv3(const float* x, int rows, int Cin, const float* w, int N, const float* bias, float* y) {
  ConvArgs a = lin(x, Cin, rows, Cin, w, N, bias, y, N);
  a.w_ts = (long long)N * Cin;
  a.taps = 3;
  a.pad = 1;
  return a;
}

int nbin_padded(int n_fft) { return (n_fft / 2 + 1 + 31) / 32 * 32; }

// librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) with its defaults htk=False, norm='slaney' (FCPE.py:123-126),
// rows of nbin_padded floats (bins past n_fft / 2 zero)
std::vector<float> mel_basis(const FcpeCfg& g) {
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  auto hz2mel = [&](double f) { return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp; };
  auto mel2hz = [&](double m) { return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m; };
  const int n = g.n_mels + 2, nbin = g.n_fft / 2 + 1, ld = nbin_padded(g.n_fft);
  const double lo = hz2mel(g.fmin), hi = hz2mel(g.fmax), step = (hi - lo) / (n - 1);
  std::vector<double> mel_f(n);
  for (int i = 0; i < n; ++i) mel_f[i] = mel2hz(i == n - 1 ? hi : lo + i * step);
  std::vector<float> w((size_t)g.n_mels * ld, 0.f);
  for (int i = 0; i < g.n_mels; ++i) {
    const double fd0 = mel_f[i + 1] - mel_f[i], fd1 = mel_f[i + 2] - mel_f[i + 1];
    const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
    for (int k = 0; k < nbin; ++k) {
      const double f = k * ((double)g.sr / g.n_fft);
      const float tri = (float)std::max(0.0, std::min(-(mel_f[i] - f) / fd0, (mel_f[i + 2] - f) / fd1));
      w[(size_t)i * ld + k] = (float)((double)tri * enorm);
    }
  }
  return w;
}

// the STFT (periodic Hann window of `win`, center = False) as a conv over 32-sample rows: W[tap][n][c], sample
// 32 tap + c; n < nbin real, else imaginary
std::vector<float> stft_weights(int win) {
  const int nbin = win / 2 + 1, taps = win / 32;
  std::vector<float> w((size_t)taps * 2 * nbin * 32);
  const double pi = 3.14159265358979323846;
  for (int t = 0; t < taps; ++t)
    for (int nn = 0; nn < 2 * nbin; ++nn)
      for (int cc = 0; cc < 32; ++cc) {
        const int k = 32 * t + cc;
        const double wn = 0.5 - 0.5 * std::cos(2.0 * pi * k / win);
        const int f = nn < nbin ? nn : nn - nbin;
        const double ang = 2.0 * pi * (double)((long long)k * f % win) / win;
        w[((size_t)t * 2 * nbin + nn) * 32 + cc] = (float)(wn * (nn < nbin ? std::cos(ang) : -std::sin(ang)));
      }
  return w;
}

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
  c.alloc_weight("fc.mel", mel_basis(g));
  c.alloc_weight("fc.stack0.w", pack_k(getf(c, "stack.0.weight", {C, g.n_mels, 3})));
  c.alloc_weight("fc.stack0.b", getf(c, "stack.0.bias", {C}).v);
  c.alloc_weight("fc.gn.g", getf(c, "stack.1.weight", {C}).v);
  c.alloc_weight("fc.gn.b", getf(c, "stack.1.bias", {C}).v);
  c.alloc_weight("fc.stack3.w", pack_k(getf(c, "stack.3.weight", {C, C, 3})));
  c.alloc_weight("fc.stack3.b", getf(c, "stack.3.bias", {C}).v);
  for (int i = 0; i < g.n_layers; ++i) {
    const std::string p = lp(i);
    c.alloc_weight(dn(i, "ln.g"), getf(c, p + "norm.weight", {C}).v);
    c.alloc_weight(dn(i, "ln.b"), getf(c, p + "norm.bias", {C}).v);
    std::vector<float> w, b;
    for (const char* n : {"to_q", "to_k", "to_v"}) {
      const auto& wv = getf(c, p + "attn." + n + ".weight", {inner, C}).v;
      const auto& bv = getf(c, p + "attn." + n + ".bias", {inner}).v;
      w.insert(w.end(), wv.begin(), wv.end());
      b.insert(b.end(), bv.begin(), bv.end());
    }
    c.alloc_weight(dn(i, "qkv.w"), w);
    c.alloc_weight(dn(i, "qkv.b"), b);
    c.alloc_weight(dn(i, "proj"), getf(c, p + "attn.fast_attention.projection_matrix", {g.n_feat, g.dim_head}).v);
    c.alloc_weight(dn(i, "out.w"), getf(c, p + "attn.to_out.weight", {C, inner}).v);
    c.alloc_weight(dn(i, "out.b"), getf(c, p + "attn.to_out.bias", {C}).v);
    c.alloc_weight(dn(i, "cf.ln.g"), getf(c, p + "conformer.net.0.weight", {C}).v);
    c.alloc_weight(dn(i, "cf.ln.b"), getf(c, p + "conformer.net.0.bias", {C}).v);
    c.alloc_weight(dn(i, "cf.pw1.w"), getf(c, p + "conformer.net.2.weight", {4 * C, C, 1}).v);
    c.alloc_weight(dn(i, "cf.pw1.b"), getf(c, p + "conformer.net.2.bias", {4 * C}).v);
    const auto& dw = getf(c, p + "conformer.net.4.conv.weight", {2 * C, 1, K}).v;
    std::vector<float> dwt((size_t)K * 2 * C);
    for (int ch = 0; ch < 2 * C; ++ch)
      for (int k = 0; k < K; ++k) dwt[(size_t)k * 2 * C + ch] = dw[(size_t)ch * K + k];
    c.alloc_weight(dn(i, "cf.dw.w"), dwt);
    c.alloc_weight(dn(i, "cf.dw.b"), getf(c, p + "conformer.net.4.conv.bias", {2 * C}).v);
    c.alloc_weight(dn(i, "cf.pw2.w"), getf(c, p + "conformer.net.6.weight", {C, 2 * C, 1}).v);
    c.alloc_weight(dn(i, "cf.pw2.b"), getf(c, p + "conformer.net.6.bias", {C}).v);
  }
  c.alloc_weight("fc.norm.g", getf(c, "norm.weight", {C}).v);
  c.alloc_weight("fc.norm.b", getf(c, "norm.bias", {C}).v);
  c.alloc_weight("fc.dense.w", getf(c, "dense_out.weight", {g.out_dims, C}).v);
  c.alloc_weight("fc.dense.b", getf(c, "dense_out.bias", {g.out_dims}).v);
  c.alloc_weight("fc.cent", getf(c, "cent_table", {g.out_dims}).v);
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
  const int nbin = g.n_fft / 2 + 1, ldm = nbin_padded(g.n_fft);
  const int64_t pl = (g.win - g.hop) / 2, pr = std::max<int64_t>((g.win - g.hop + 1) / 2, g.win - n - pl);
  const int64_t np = n + pl + pr, rows = (np + 31) / 32;
  const int Fs = (int)((np - g.win) / g.hop + 1);
  const int F = (int)fcpe_frames(c, n), Fm = std::min(Fs, F);
  if ((int64_t)B * F > INT32_MAX / std::max(4 * g.n_chans, 2 * nbin)) throw Error(RVCX_E_SHAPE, "fcpe: too many frames");
  float* xp = c.buf<float>("fc.xp", (size_t)B * rows * 32, s);
  if (pr < n) {
    check(reflect_pad_1d(audio, (int)n, (int)pl, (int)pr, xp, s, B, ld, rows * 32), "fcpe_pad");
  } else {  // torch pads with zeros when the reflection would not fit (:138)
    check(fcpe_zero_pad(audio, (int)n, (int)pl, ld, xp, rows * 32, B, s), "fcpe_pad");
  }
  float* spec = c.buf<float>("fc.spec", (size_t)B * Fm * 2 * nbin, s);
  {
    ConvArgs a = lin(xp, 32, (int)rows, 32, c.W("fc.stft"), 2 * nbin, nullptr, spec, 2 * nbin);
    a.taps = g.win / 32;
    a.stride = g.hop / 32;
    a.w_ts = (long long)2 * nbin * 32;
    a.T_out = Fm;
    a.batch = B;
    a.x_bs = rows * 32;
    a.y_bs = (long long)Fm * 2 * nbin;
    launch_conv(c, a, false, s, 0.0);
  }
  float* mag = c.buf<float>("fc.mag", (size_t)B * Fm * ldm, s);
  check(fcpe_magnitude(spec, B * Fm, nbin, mag, ldm, s), "fcpe_magnitude");
  {
    ConvArgs a = lin(mag, ldm, Fm, ldm, c.W("fc.mel"), g.n_mels, nullptr, mel, g.n_mels);
    a.act = ACT_LOGCLAMP;
    a.slope = 1e-5f;
    a.batch = B;  // Fm rows of each stream into its F rows of mel
    a.x_bs = (long long)Fm * ldm;
    a.y_bs = (long long)F * g.n_mels;
    launch_conv(c, a, false, s);
  }
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
  auto per_stream = [&](ConvArgs a, int Cin, int N) {  // a k = 3 conv over each stream's own F rows
    a.batch = B;
    a.x_bs = (long long)F * Cin;
    a.y_bs = (long long)F * N;
    return a;
  };
  // ---- input stack (:624-631)
  float* x = c.buf<float>("fc.x", (size_t)R * C, s);
  float* x1 = c.buf<float>("fc.x1", (size_t)R * C, s);
  float* ln = c.buf<float>("fc.ln", (size_t)R * C, s);
  launch_conv(c, per_stream(conv3(mel, F, g.n_mels, c.W("fc.stack0.w"), C, c.W("fc.stack0.b"), x1), g.n_mels, C), false,
              s);
  double* gnws = c.buf<double>("fc.gnws", (size_t)B * 4 * FCPE_GN_CHUNKS * 2, s);
  check(groupnorm_lrelu(x1, F, C, 4, c.W("fc.gn.g"), c.W("fc.gn.b"), 1e-5f, 0.01f, gnws, s, B), "fcpe_groupnorm");
  launch_conv(c, per_stream(conv3(x1, F, C, c.W("fc.stack3.w"), C, c.W("fc.stack3.b"), x), C, C), false, s);
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
