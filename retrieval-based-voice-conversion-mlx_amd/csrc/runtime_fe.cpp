// Front end of the pipeline on device: HuBERT/ContentVec features and the RMVPE pitch predictor.
//   HuBERT: transformers modeling_hubert.py HubertModel (contentvec config:
//           rvc_mlx/models/embedders/contentvec/config.json); MLX rvc_mlx/lib/mlx/hubert.py.
//   RMVPE : rvc/lib/predictors/RMVPE.py (E2E U-Net + BiGRU, MelSpectrogram, decode);
//           MLX rvc_mlx/lib/mlx/rmvpe.py.
#include <cmath>
#include <utility>

#include "model_build.h"
#include "rows.h"

namespace rvcx {

namespace {

constexpr int HD = 768, HHEADS = 12, HFF = 3072, HCONV = 512;
const int HK[7] = {10, 3, 3, 3, 3, 2, 2};
const int HS[7] = {5, 2, 2, 2, 2, 2, 2};
constexpr int POS_K = 128, POS_G = 16;

}  // namespace

// ================================================================== HuBERT
void finalize_hubert(Ctx& c) {
  const int M = 1;
  // conv0 (C_in 1, k 10, s 5): [512][1][10] as is, the fused conv + GroupNorm + GELU kernel's [c][k] layout
  c.alloc_weight("hb.conv0", host_weight(c, M, "feature_extractor.conv_layers.0.conv.weight", {HCONV, 1, HK[0]}).v);
  for (int i = 1; i < 7; ++i)
    c.alloc_weight("hb.conv" + std::to_string(i),
                   pack_conv1d(host_weight(c, M, "feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight",
                                    {HCONV, HCONV, HK[i]})));
  c.alloc_weight("hb.gn.g", host_weight(c, M, "feature_extractor.conv_layers.0.layer_norm.weight", {HCONV}).v);
  c.alloc_weight("hb.gn.b", host_weight(c, M, "feature_extractor.conv_layers.0.layer_norm.bias", {HCONV}).v);
  c.alloc_weight("hb.fp.ln.g", host_weight(c, M, "feature_projection.layer_norm.weight", {HCONV}).v);
  c.alloc_weight("hb.fp.ln.b", host_weight(c, M, "feature_projection.layer_norm.bias", {HCONV}).v);
  c.alloc_weight("hb.fp.w", host_weight(c, M, "feature_projection.projection.weight", {HD, HCONV}).v);
  c.alloc_weight("hb.fp.b", host_weight(c, M, "feature_projection.projection.bias", {HD}).v);
  {  // grouped positional conv: [768][48][128] -> [group][tap][48 out][48 in]
    const int cg = HD / POS_G;
    auto& w = host_weight(c, M, "encoder.pos_conv_embed.conv.weight", {HD, cg, POS_K});
    std::vector<float> v((size_t)POS_G * POS_K * cg * cg);
    for (int g = 0; g < POS_G; ++g)
      for (int t = 0; t < POS_K; ++t)
        for (int o = 0; o < cg; ++o)
          for (int i = 0; i < cg; ++i)
            v[(((size_t)g * POS_K + t) * cg + o) * cg + i] = w.v[((size_t)(g * cg + o) * cg + i) * POS_K + t];
    c.alloc_weight("hb.pos.w", v);
    c.alloc_weight("hb.pos.b", host_weight(c, M, "encoder.pos_conv_embed.conv.bias", {HD}).v);
  }
  c.alloc_weight("hb.enc.ln.g", host_weight(c, M, "encoder.layer_norm.weight", {HD}).v);
  c.alloc_weight("hb.enc.ln.b", host_weight(c, M, "encoder.layer_norm.bias", {HD}).v);
  for (int i = 0; i < 12; ++i) {
    const std::string p = "encoder.layers." + std::to_string(i);
    const std::string q = "hb." + std::to_string(i);
    std::vector<float> w, b;
    for (const char* n : {"q_proj", "k_proj", "v_proj"}) {
      auto& tw = host_weight(c, M, p + ".attention." + n + ".weight", {HD, HD}).v;
      auto& tb = host_weight(c, M, p + ".attention." + n + ".bias", {HD}).v;
      w.insert(w.end(), tw.begin(), tw.end());
      b.insert(b.end(), tb.begin(), tb.end());
    }
    c.alloc_weight(q + ".qkv.w", w);
    c.alloc_weight(q + ".qkv.b", b);
    c.alloc_weight(q + ".o.w", host_weight(c, M, p + ".attention.out_proj.weight", {HD, HD}).v);
    c.alloc_weight(q + ".o.b", host_weight(c, M, p + ".attention.out_proj.bias", {HD}).v);
    c.alloc_weight(q + ".ln1.g", host_weight(c, M, p + ".layer_norm.weight", {HD}).v);
    c.alloc_weight(q + ".ln1.b", host_weight(c, M, p + ".layer_norm.bias", {HD}).v);
    c.alloc_weight(q + ".ff1.w", host_weight(c, M, p + ".feed_forward.intermediate_dense.weight", {HFF, HD}).v);
    c.alloc_weight(q + ".ff1.b", host_weight(c, M, p + ".feed_forward.intermediate_dense.bias", {HFF}).v);
    c.alloc_weight(q + ".ff2.w", host_weight(c, M, p + ".feed_forward.output_dense.weight", {HD, HFF}).v);
    c.alloc_weight(q + ".ff2.b", host_weight(c, M, p + ".feed_forward.output_dense.bias", {HD}).v);
    c.alloc_weight(q + ".ln2.g", host_weight(c, M, p + ".final_layer_norm.weight", {HD}).v);
    c.alloc_weight(q + ".ln2.b", host_weight(c, M, p + ".final_layer_norm.bias", {HD}).v);
  }
  if (c.host[M].count("final_proj.weight")) {
    c.alloc_weight("hb.final_proj.w", host_weight(c, M, "final_proj.weight", {256, HD}).v);
    c.alloc_weight("hb.final_proj.b", host_weight(c, M, "final_proj.bias", {256}).v);
  }
}

int64_t hubert_frames(int64_t n) {
  int64_t t = n;
  for (int i = 0; i < 7; ++i) {
    if (t < HK[i]) return 0;
    t = (t - HK[i]) / HS[i] + 1;
  }
  return t;
}

// B sequences: audio row b at audio + b*lda; feats row block b at feats + b*L*outD.
// Row-wise ops (LayerNorm, Linear, FFN) run over all B*L rows at once; convolutions, GroupNorm and
// attention take the sequence as their batch index.
// nv == nullptr: B equal-length sequences of n samples. nv[B] (host): sequence b has nv[b] <= n samples and L is the
// longest one's frame count. A sequence's frames are then those of a run on it alone, up to summation order:
//   - conv0's GroupNorm statistics are over the sequence's own frames, and its frames past them are written as zero;
//   - the strided convs are valid convolutions, so a sequence's valid frames read only its valid inputs (its pad
//     frames read zeros and the tail of the valid ones: finite, and never read by a valid frame);
//   - the feature projection writes pad frames as zero, which is the zero padding the positional conv (k 128, pad 64)
//     reads past a sequence's end;
//   - attention masks the pad keys (run.mask); every other op is row-wise.
static HubertRun front(Ctx& c, const float* audio, int64_t n, const int64_t* nv, int64_t lda, int B, int version,
                       float* feats, int64_t cap, hipStream_t s, int lds_pad = 0) {
  if (B < 1) throw Error(RVCX_E_INVALID, "hubert: batch < 1");
  int64_t T[8];
  T[0] = n;
  for (int i = 0; i < 7; ++i) {
    if (T[i] < HK[i]) throw Error(RVCX_E_SHAPE, "hubert: input too short (" + std::to_string(n) + " samples)");
    T[i + 1] = (T[i] - HK[i]) / HS[i] + 1;
  }
  const int L = (int)T[7];
  const int BL = B * L;
  if (L > cap) throw Error(RVCX_E_CAPACITY, "hubert: output needs " + std::to_string(L) + " rows");
  float* a = c.buf<float>("hb.a", (size_t)B * T[1] * HCONV, s);
  float* b = c.buf<float>("hb.b", (size_t)B * T[2] * HCONV, s);
  double* gnws = c.buf<double>("hb.gnws", groupnorm_ws_doubles(HCONV, B), s);
  float* mask = nullptr;
  Len T1((int)T[1]);  // conv0 frames per sequence
  if (nv) {
    // per-sequence conv0 frames | output frames on device, and the [B][L] mask of valid output frames
    LenCols len(2, B);
    for (int r = 0; r < B; ++r) {
      const int64_t Lr = hubert_frames(nv[r]);
      if (Lr < 1) throw Error(RVCX_E_SHAPE, "hubert: input too short (" + std::to_string(nv[r]) + " samples)");
      len.at(0, r) = (int32_t)((nv[r] - HK[0]) / HS[0] + 1);
      len.at(1, r) = (int32_t)Lr;
    }
    len.upload(c, "hb.lens", s);
    mask = c.buf<float>("hb.mask", (size_t)BL, s);
    check(seq_mask(len.col(1), mask, B, L, s), "hubert_mask");
    T1 = Len(len.col(0));
  }
  // conv0 -> GroupNorm(512, 512) -> GELU in three launches (statistics, finalize, apply), the conv recomputed by each
  check(hubert_conv0_gn_gelu(audio, lda, c.W("hb.conv0"), T1, (int)T[1], HCONV, c.W("hb.gn.g"), c.W("hb.gn.b"), 1e-5f,
                             gnws, a, s, B),
        "hubert_conv0");
  float* cur = a;
  float* nxt = b;
  for (int i = 1; i < 7; ++i) {
    ConvArgs ci = lin(cur, HCONV, (int)T[i], HCONV, c.W("hb.conv" + std::to_string(i)), HCONV, nullptr, nxt, HCONV);
    ci.taps = HK[i];
    ci.stride = HS[i];
    ci.w_ts = (long long)HCONV * HCONV;
    ci.T_out = (int)T[i + 1];
    ci.act = ACT_GELU;
    ci.batch = B;
    ci.x_bs = T[i] * HCONV;
    ci.y_bs = T[i + 1] * HCONV;
    ci.lds_pad = lds_pad;
    run1(c, ci, s);
    std::swap(cur, nxt);
  }
  // feature projection: LayerNorm(512) -> Linear(512, 768)
  float* hs = c.buf<float>("hb.hs", (size_t)BL * HD, s);
  float* hs2 = c.buf<float>("hb.hs2", (size_t)BL * HD, s);
  check(layernorm_rows(cur, nullptr, nxt, c.W("hb.fp.ln.g"), c.W("hb.fp.ln.b"), BL, HCONV, 1e-5f, nullptr, s),
        "fp_ln");
  {
    ConvArgs fp = lin(nxt, HCONV, BL, HCONV, c.W("hb.fp.w"), HD, c.W("hb.fp.b"), hs, HD);
    fp.mask = mask;  // ragged: pad frames become the positional conv's zero padding
    fp.lds_pad = lds_pad;
    run1(c, fp, s);
  }
  {  // hs + gelu(pos_conv(hs)) (groups as inner batch, sequences as outer batch), then encoder LayerNorm
    const int cg = HD / POS_G;
    ConvArgs p = lin(hs, HD, L, cg, c.W("hb.pos.w"), cg, c.W("hb.pos.b"), hs2, HD);
    p.taps = POS_K;
    p.pad = POS_K / 2;
    p.ldw = cg;
    p.w_ts = (long long)cg * cg;
    p.batch_inner = POS_G;
    p.x_bs2 = cg;
    p.w_bs2 = (long long)POS_K * cg * cg;
    p.y_bs2 = cg;
    p.bias_bs2 = cg;
    p.act = ACT_GELU;
    p.res = hs;
    p.ldr = HD;
    p.res_bs2 = cg;
    p.res_mode = RES_ADD_POST;
    p.batch = B;
    p.x_bs = p.y_bs = p.res_bs = (long long)L * HD;
    p.lds_pad = lds_pad;
    run1(c, p, s);
    check(layernorm_rows(hs2, nullptr, hs, c.W("hb.enc.ln.g"), c.W("hb.enc.ln.b"), BL, HD, 1e-5f, nullptr, s),
          "enc_ln");
  }
  HubertRun r;
  r.B = B;
  r.L = L;
  r.version = version;
  r.feats = feats;
  r.mask = mask;
  r.lds_pad = lds_pad;
  return r;
}

HubertRun hubert_front(Ctx& c, const float* audio, int64_t n, int64_t lda, int B, int version, float* feats,
                       int64_t cap, hipStream_t s, int lds_pad) {
  return front(c, audio, n, nullptr, lda, B, version, feats, cap, s, lds_pad);
}

// encoder layers [l0, l1) on the hidden states the front end left in "hb.hs" (modeling_hubert.py
// HubertEncoderLayer: post-LN attention + FFN)
void hubert_layers(Ctx& c, const HubertRun& run, int l0, int l1, hipStream_t s) {
  const int B = run.B, L = run.L, BL = B * L;
  float* hs = c.buf<float>("hb.hs", (size_t)BL * HD, s);
  float* qkv = c.buf<float>("hb.qkv", (size_t)BL * 3 * HD, s);
  const int nsplit = flash_attn_splits(B, HHEADS, L);
  float* part_o = c.buf<float>("hb.fa_o", (size_t)flash_attn_ws_floats(B, HHEADS, L, HD / HHEADS, nsplit), s);
  float* part_ml = c.buf<float>("hb.fa_ml", (size_t)nsplit * B * HHEADS * L * 2, s);
  float* att = c.buf<float>("hb.att", (size_t)BL * HD, s);
  float* ff = c.buf<float>("hb.ff", (size_t)BL * HFF, s);
  const int hd = HD / HHEADS;
  for (int i = l0; i < l1; ++i) {
    const std::string q = "hb." + std::to_string(i);
    {
      ConvArgs a1 = lin(hs, HD, BL, HD, c.W(q + ".qkv.w"), 3 * HD, c.W(q + ".qkv.b"), qkv, 3 * HD);
      a1.lds_pad = run.lds_pad;
      run1(c, a1, s);
    }
    // softmax((q * hd^-0.5) k^T) v per head in one pass (flash_attn.hip): no [B][12][L][L] scores. Ragged batches
    // (run.mask): a pad key's score is -1e4, which is exp(-1e4 - max) == 0 in fp32 beside any valid key's (the scores
    // of LayerNormed rows are far inside +-9e3), so it adds exactly 0 to a valid query's sums
    check(flash_attn(qkv, 3 * HD, B, L, HHEADS, hd, (float)std::pow((double)hd, -0.5), nullptr, nullptr, 0, run.mask,
                     part_o, part_ml, nsplit, att, HD, s),
          "flash_attn");
    {  // hs = LN(hs + out_proj(att)) (layer_norm) in the split-K combine, in place: one combine block per row reads
       // the row's residual before it writes the row (round 6: the combine + a separate LayerNorm pass before)
      ConvArgs a3 = lin(att, HD, BL, HD, c.W(q + ".o.w"), HD, c.W(q + ".o.b"), hs, HD);
      a3.res = hs;
      a3.ldr = HD;
      a3.ln_g = c.W(q + ".ln1.g");
      a3.ln_b = c.W(q + ".ln1.b");
      a3.lds_pad = run.lds_pad;
      run1(c, a3, s);
    }
    {
      ConvArgs f1 = lin(hs, HD, BL, HD, c.W(q + ".ff1.w"), HFF, c.W(q + ".ff1.b"), ff, HFF);
      f1.act = ACT_GELU;
      f1.lds_pad = run.lds_pad;
      run1(c, f1, s);
      // v2's output is the last layer's LN itself: written straight into the caller's buffer (no tail copy)
      float* dst = (run.version != 1 && i == HUBERT_LAYERS - 1) ? run.feats : hs;
      // dst = LN(hs + ff2(ff)) in the split-K combine (final_layer_norm): no hs2 round trip, no separate pass
      ConvArgs f2 = lin(ff, HFF, BL, HFF, c.W(q + ".ff2.w"), HD, c.W(q + ".ff2.b"), dst, HD);
      f2.res = hs;
      f2.ldr = HD;
      f2.ln_g = c.W(q + ".ln2.g");
      f2.ln_b = c.W(q + ".ln2.b");
      f2.lds_pad = run.lds_pad;
      run1(c, f2, s);
    }
  }
}

// v2: last_hidden_state; v1: final_proj (pipeline.py:331-334)
int64_t hubert_tail(Ctx& c, const HubertRun& run, hipStream_t s) {
  const int BL = run.B * run.L;
  const int version = run.version;
  float* hs = c.buf<float>("hb.hs", (size_t)BL * HD, s);
  float* feats = run.feats;
  if (version == 1) {
    if (!c.dev.count("hb.final_proj.w")) throw Error(RVCX_E_STATE, "hubert: v1 needs final_proj weights");
    ConvArgs fp = lin(hs, HD, BL, HD, c.W("hb.final_proj.w"), 256, c.W("hb.final_proj.b"), feats, 256);
    fp.lds_pad = run.lds_pad;
    run1(c, fp, s);
  }  // v2: the last layer wrote feats (hubert_layers)
  return run.L;
}

int64_t hubert_forward_b(Ctx& c, const float* audio, int64_t n, int64_t lda, int B, int version, float* feats,
                         int64_t cap, hipStream_t s) {
  const HubertRun r = hubert_front(c, audio, n, lda, B, version, feats, cap, s);
  hubert_layers(c, r, 0, HUBERT_LAYERS, s);
  return hubert_tail(c, r, s);
}

int64_t hubert_forward(Ctx& c, const float* audio, int64_t n, int version, float* feats, int64_t cap,
                       hipStream_t s) {
  return hubert_forward_b(c, audio, n, n, 1, version, feats, cap, s);
}

// (runtime.h) The rows of a sequence past its L_b, up to the longest's, are written and hold no meaning.
int64_t hubert_forward_v(Ctx& c, const float* audio, const int64_t* nv, int64_t lda, int B, int version, float* feats,
                         int64_t ld_rows, int64_t* rows_out, hipStream_t s, bool force_ragged) {
  const Rows r("hubert", nv, B, lda);
  const int64_t L = hubert_frames(r.n_max);
  if (L > ld_rows) throw Error(RVCX_E_CAPACITY, "hubert: output needs " + std::to_string(L) + " rows per sequence");
  const int outD = version == 1 ? 256 : HD;
  // the layers write [B][L][outD] back to back: straight into the caller's rows when their stride is L
  const Staged<float> dst(c, "hb.featv", feats, ld_rows * outD, L * outD, B, s);
  // equal lengths need no masks: the equal-length form, bit for bit
  const HubertRun run = front(c, audio, r.n_max, r.equal && !force_ragged ? nullptr : nv, lda, B, version, dst.p, L, s);
  hubert_layers(c, run, 0, HUBERT_LAYERS, s);
  hubert_tail(c, run, s);
  dst.copy_out(s);
  if (rows_out)
    for (int b = 0; b < B; ++b) rows_out[b] = hubert_frames(nv[b]);
  return L;
}

// ================================================================== RMVPE
namespace {

constexpr int NMEL = 128, NFFT = 1024, HOP = 160, NBIN = NFFT / 2 + 1, NCLS = 360;
// the mel projection's contraction padded to whole 32-bin chunks (zero magnitudes x zero weights): K = 513 kept it off
// the streamed fp16 kernels (the three-plane LDS kernel + a split-K combine: 60 + 16 us at C2, r05i)
constexpr int NBIN_P = 544;
constexpr int LEVELS = 5, INTER = 4, NBLK = 4, C_BASE = 16, GRU_H = 256;
// MelSpectrogram (RMVPE.py:388-417): librosa's htk=True basis from 30 Hz to 8 kHz, plain |STFT|
constexpr MelSpec MEL{16000, NFFT, HOP, NMEL, 30.0, 8000.0, true, 0.f};
static_assert(MEL.nbin() == NBIN && MEL.ld() == NBIN_P, "the mel rows are NBIN_P floats");

struct BN {
  std::vector<double> a, b;
};
BN bn_fold(Ctx& c, const std::string& p, int C) {
  auto& g = host_weight(c, 2, p + ".weight", {C}).v;
  auto& bb = host_weight(c, 2, p + ".bias", {C}).v;
  auto& m = host_weight(c, 2, p + ".running_mean", {C}).v;
  auto& v = host_weight(c, 2, p + ".running_var", {C}).v;
  BN r;
  r.a.resize(C);
  r.b.resize(C);
  for (int i = 0; i < C; ++i) {
    const double inv = 1.0 / std::sqrt((double)v[i] + 1e-5);
    r.a[i] = inv * g[i];
    r.b[i] = (double)bb[i] - (double)m[i] * r.a[i];
  }
  return r;
}

// Conv2d [O][I][3][3] + BN -> [9][O][I], bias [O]
void conv_bn(Ctx& c, const std::string& wname, const std::string& bnname, int O, int I, const std::string& dst) {
  auto& w = host_weight(c, 2, wname, {O, I, 3, 3}).v;
  BN bn = bn_fold(c, bnname, O);
  std::vector<float> v((size_t)9 * O * I), bias(O);
  for (int o = 0; o < O; ++o) {
    for (int i = 0; i < I; ++i)
      for (int t = 0; t < 9; ++t) v[((size_t)t * O + o) * I + i] = (float)((double)w[((size_t)o * I + i) * 9 + t] * bn.a[o]);
    bias[o] = (float)bn.b[o];
  }
  c.alloc_weight(dst + ".w", v);
  c.alloc_weight(dst + ".b", bias);
}

void block_weights(Ctx& c, const std::string& p, const std::string& q, int cin, int cout) {
  conv_bn(c, p + ".conv.0.weight", p + ".conv.1", cout, cin, q + ".c1");
  conv_bn(c, p + ".conv.3.weight", p + ".conv.4", cout, cout, q + ".c2");
  if (cin != cout) {
    c.alloc_weight(q + ".sc.w", host_weight(c, 2, p + ".shortcut.weight", {cout, cin, 1, 1}).v);
    c.alloc_weight(q + ".sc.b", host_weight(c, 2, p + ".shortcut.bias", {cout}).v);
  }
}

ConvArgs c2d(const float* x, int ldx, int H, int W, int Cin, const float* w, int N, const float* bias, float* y,
             int ldy, int B = 1, const int* hv = nullptr) {
  ConvArgs a = lin(x, ldx, H, Cin, w, N, bias, y, ldy);  // rows = image rows
  a.batch = B;  // B images of H x W pixels back to back
  a.h_in = hv;  // image b's own rows (device, optional): the conv zero-pads at its own last row
  a.x_bs = (long long)H * W * ldx;
  a.y_bs = (long long)H * W * ldy;
  a.W_in = a.W_out = W;
  a.w_ts = (long long)N * Cin;
  a.taps = 9;
  a.KH = a.KW = 3;
  a.padh = a.padw = 1;
  return a;
}

// ConvBlockRes (RMVPE.py:13-57): relu(bn(conv)) x2 + shortcut(x) (or x)
// B images back to back (NHWC, row stride ldx / ldy per pixel)
void conv_block(Ctx& c, const std::string& q, const float* x, int ldx, int H, int W, int cin, int cout, float* y,
                int ldy, hipStream_t s, int B = 1, const int* hv = nullptr) {
  const size_t P = (size_t)H * W;
  float* t = c.buf<float>("rm.blk.t", (size_t)B * P * cout, s);
  ConvArgs a = c2d(x, ldx, H, W, cin, c.W(q + ".c1.w"), cout, c.W(q + ".c1.b"), t, cout, B, hv);
  a.act = ACT_RELU;
  run2(c, a, s);
  const float* res = x;
  int ldr = ldx;
  if (cin != cout) {
    float* sc = c.buf<float>("rm.blk.sc", (size_t)B * P * cout, s);
    run1(c, lin(x, ldx, (int)(B * P), cin, c.W(q + ".sc.w"), cout, c.W(q + ".sc.b"), sc, cout), s);
    res = sc;
    ldr = cout;
  }
  ConvArgs b = c2d(t, cout, H, W, cout, c.W(q + ".c2.w"), cout, c.W(q + ".c2.b"), y, ldy, B, hv);
  b.act = ACT_RELU;
  b.res = res;
  b.ldr = ldr;
  b.res_bs = (long long)P * ldr;
  b.res_mode = RES_ADD_POST;
  run2(c, b, s);
}

}  // namespace

void finalize_rmvpe(Ctx& c) {
  c.alloc_weight("rm.stft", stft_weights(MEL.win));
  c.alloc_weight("rm.mel", mel_basis(MEL));
  {
    BN bn = bn_fold(c, "unet.encoder.bn", 1);
    c.host[2]["__bn0__"] = HostTensor{{(float)bn.a[0], (float)bn.b[0]}, {2}};
  }
  int cin = 1, cout = C_BASE;
  for (int i = 0; i < LEVELS; ++i) {
    for (int b = 0; b < NBLK; ++b)
      block_weights(c, "unet.encoder.layers." + std::to_string(i) + ".conv." + std::to_string(b),
                    "rm.enc" + std::to_string(i) + "." + std::to_string(b), b == 0 ? cin : cout, cout);
    cin = cout;
    cout *= 2;
  }
  const int top = C_BASE << LEVELS;  // 512
  int ci = top / 2;
  for (int i = 0; i < INTER; ++i) {
    for (int b = 0; b < NBLK; ++b)
      block_weights(c, "unet.intermediate.layers." + std::to_string(i) + ".conv." + std::to_string(b),
                    "rm.int" + std::to_string(i) + "." + std::to_string(b), b == 0 ? ci : top, top);
    ci = top;
  }
  int C = top;
  for (int i = 0; i < LEVELS; ++i) {
    const int co = C / 2;
    const std::string p = "unet.decoder.layers." + std::to_string(i);
    const std::string q = "rm.dec" + std::to_string(i);
    {  // ConvTranspose2d 3x3 s2 p1 op1 + BN as a 2x2-tap phase conv with 4*co virtual outputs
      auto& w = host_weight(c, 2, p + ".conv1.0.weight", {C, co, 3, 3}).v;
      BN bn = bn_fold(c, p + ".conv1.1", co);
      std::vector<float> v((size_t)4 * 4 * co * C, 0.f), bias((size_t)4 * co);
      const int kmap[2][2] = {{1, -1}, {2, 0}};  // [phase][input offset] -> kernel index
      for (int dh = 0; dh < 2; ++dh)
        for (int dw = 0; dw < 2; ++dw)
          for (int ph = 0; ph < 2; ++ph)
            for (int pw = 0; pw < 2; ++pw) {
              const int kh = kmap[ph][dh], kw = kmap[pw][dw];
              if (kh < 0 || kw < 0) continue;
              const int tap = dh * 2 + dw;
              for (int o = 0; o < co; ++o) {
                const int n = (ph * 2 + pw) * co + o;
                for (int ii = 0; ii < C; ++ii)
                  v[((size_t)tap * 4 * co + n) * C + ii] =
                      (float)((double)w[(((size_t)ii * co + o) * 3 + kh) * 3 + kw] * bn.a[o]);
              }
            }
      for (int ph = 0; ph < 4; ++ph)
        for (int o = 0; o < co; ++o) bias[(size_t)ph * co + o] = (float)bn.b[o];
      c.alloc_weight(q + ".up.w", v);
      c.alloc_weight(q + ".up.b", bias);
    }
    for (int b = 0; b < NBLK; ++b)
      block_weights(c, p + ".conv2." + std::to_string(b), q + "." + std::to_string(b), b == 0 ? 2 * co : co, co);
    C = co;
  }
  c.alloc_weight("rm.cnn.w", [&] {
    auto& w = host_weight(c, 2, "cnn.weight", {3, C_BASE, 3, 3}).v;
    std::vector<float> v((size_t)9 * 3 * C_BASE);
    for (int o = 0; o < 3; ++o)
      for (int i = 0; i < C_BASE; ++i)
        for (int t = 0; t < 9; ++t) v[((size_t)t * 3 + o) * C_BASE + i] = w[((size_t)o * C_BASE + i) * 9 + t];
    return v;
  }());
  c.alloc_weight("rm.cnn.b", host_weight(c, 2, "cnn.bias", {3}).v);
  {
    const int nin = 3 * NMEL;
    auto& wf = host_weight(c, 2, "fc.0.gru.weight_ih_l0", {3 * GRU_H, nin}).v;
    auto& wb = host_weight(c, 2, "fc.0.gru.weight_ih_l0_reverse", {3 * GRU_H, nin}).v;
    c.alloc_weight("rm.gru.wih", cat({&wf, &wb}));
    auto& bf = host_weight(c, 2, "fc.0.gru.bias_ih_l0", {3 * GRU_H}).v;
    auto& bb = host_weight(c, 2, "fc.0.gru.bias_ih_l0_reverse", {3 * GRU_H}).v;
    c.alloc_weight("rm.gru.bih", cat({&bf, &bb}));
    c.alloc_weight("rm.gru.whh_f", host_weight(c, 2, "fc.0.gru.weight_hh_l0", {3 * GRU_H, GRU_H}).v);
    c.alloc_weight("rm.gru.whh_b", host_weight(c, 2, "fc.0.gru.weight_hh_l0_reverse", {3 * GRU_H, GRU_H}).v);
    c.alloc_weight("rm.gru.bhh_f", host_weight(c, 2, "fc.0.gru.bias_hh_l0", {3 * GRU_H}).v);
    c.alloc_weight("rm.gru.bhh_b", host_weight(c, 2, "fc.0.gru.bias_hh_l0_reverse", {3 * GRU_H}).v);
  }
  c.alloc_weight("rm.fc.w", host_weight(c, 2, "fc.1.weight", {NCLS, 2 * GRU_H}).v);
  c.alloc_weight("rm.fc.b", host_weight(c, 2, "fc.1.bias", {NCLS}).v);
}

// The BiGRU recurrence of B sequences of T steps on the context's hand-off buffer (gi [B][T][1536] -> out [B][T][512]):
// the buffer and its zeroing, one tag counter per 16-sequence slice, and the launches. tag_start < 0: the counters run
// on from the earlier launches on this buffer (RMVPE); tag_start >= 0 (rvcx_gru_bidir, the tests): the buffer is
// zeroed and every slice's counter set to it first, so no granule left by an earlier launch can carry a tag this one
// waits for. Tv (device, optional): sequence b runs Tv[b] <= T steps in rows of stride T. beside_gru (optional): work
// the caller wants to go out beside the BiGRU, issued from here.
void gru_bidir_run(Ctx& c, const float* gi, int B, int T, const float* whh_f, const float* bhh_f, const float* whh_b,
                   const float* bhh_b, float* out, long long tag_start, hipStream_t s, const int* Tv,
                   const GruHook& beside_gru) {
  unsigned long long* xchg = c.buf<unsigned long long>("rm.xchg", gru_xchg_words(B), s);
  // a new (or regrown) allocation holds garbage tags: zeroed once, and the tag counters of its slices restart
  if (c.zero_once("rm.xchg", xchg, sizeof(unsigned long long) * gru_xchg_words(B), (long long)B, s))
    c.gru_tags.clear();
  if (tag_start >= 0) {
    if (tag_start > 0) RVCX_HIP(hipMemsetAsync(xchg, 0, sizeof(unsigned long long) * gru_xchg_words(B), s));
    for (int g0 = 0; g0 < B; g0 += 16) c.gru_tags[xchg + gru_xchg_words(g0)] = (unsigned)tag_start;
  }
  unsigned* status = c.device_status();  // sticky until the host reads it (Ctx::check_device_status)
  // work the caller wants issued beside the BiGRU (which occupies 4 CUs): the gate event marks this point of the
  // stream, the BiGRU goes out first and the hook's (many) launches after it, so the host time spent issuing
  // them overlaps the BiGRU instead of delaying its launch
  if (beside_gru && c.ev_gate) RVCX_HIP(hipEventRecord(c.ev_gate, s));
  for (int g0 = 0; g0 < B; g0 += 16)  // at most 16 sequences per launch (16 x 4 working workgroups co-resident)
    check(gru_bidir(gi + (size_t)g0 * T * 6 * GRU_H, whh_f, bhh_f, whh_b, bhh_b, T, out + (size_t)g0 * T * 2 * GRU_H,
                    xchg + gru_xchg_words(g0), status, &c.gru_tags[xchg + gru_xchg_words(g0)], s, std::min(16, B - g0),
                    Tv ? Tv + g0 : nullptr),
          "gru");
  if (beside_gru) beside_gru(s);
}

// E2E on B mel chunk images [B][Fc][128] (already padded to a multiple of 32 frames) -> sal [B][Fc][360].
// Pooling and the per-row transforms run on the B images stacked along time (every level's height is
// even, so no 2x2 window straddles two images); convolutions take the image as their batch index.
// hv (device, optional; row l of ldh ints: the images' own heights at level l, Fp_b >> l): images of different heights,
// each a multiple of 32 frames of its Fc rows. Every 3x3 conv and up-conv then reads zero at an image's rows from its
// own height on (ConvArgs::h_in), which is the zero padding a pass on that image alone has there, and the BiGRU runs
// each sequence over its own frames; pooling, the 1x1 shortcuts, the layout change and the linears are row-wise. An
// image's rows past its own height hold no meaning at any stage and no valid row reads them.
// beside_gru: GruHook (runtime.h), issued beside this pass's BiGRU.
static void e2e_chunk(Ctx& c, float* img, int Fc, float* sal, hipStream_t s, const GruHook& beside_gru, int B = 1,
                      const int* hv = nullptr, int ldh = 0) {
  auto hl = [&](int level) { return hv ? hv + (size_t)level * ldh : nullptr; };
  int H = Fc, W = NMEL;
  // encoder: level outputs go to the second half of the decoder concat buffers
  float* catb[LEVELS];
  int cin = 1, cout = C_BASE;
  const float* x = img;
  int ldx = 1;
  for (int i = 0; i < LEVELS; ++i) {
    catb[i] = c.buf<float>("rm.cat" + std::to_string(i), (size_t)B * H * W * 2 * cout, s);
    float* pa = c.buf<float>("rm.pa", (size_t)B * Fc * NMEL * C_BASE * 2, s);
    float* pb = c.buf<float>("rm.pb", (size_t)B * Fc * NMEL * C_BASE * 2, s);
    const float* in = x;
    int ldi = ldx, ci = cin;
    for (int b = 0; b < NBLK; ++b) {
      const bool last = b == NBLK - 1;
      float* out = last ? catb[i] + cout : (b % 2 == 0 ? pa : pb);
      conv_block(c, "rm.enc" + std::to_string(i) + "." + std::to_string(b), in, ldi, H, W, ci, cout, out,
                 last ? 2 * cout : cout, s, B, hl(i));
      in = out;
      ldi = last ? 2 * cout : cout;
      ci = cout;
    }
    float* pooled = c.buf<float>("rm.pool" + std::to_string(i), (size_t)B * (H / 2) * (W / 2) * cout, s);
    check(avgpool2(catb[i] + cout, B * H, W, cout, 2 * cout, pooled, s), "avgpool");
    x = pooled;
    ldx = cout;
    H /= 2;
    W /= 2;
    cin = cout;
    cout *= 2;
  }
  // intermediate (4 x ResEncoderBlock without pooling)
  const int top = C_BASE << LEVELS;
  {
    float* ia = c.buf<float>("rm.ia", (size_t)B * H * W * top, s);
    float* ib = c.buf<float>("rm.ib", (size_t)B * H * W * top, s);
    const float* in = x;
    int ci = cin, ldi = ldx, k = 0;
    for (int i = 0; i < INTER; ++i)
      for (int b = 0; b < NBLK; ++b, ++k) {
        float* out = (k % 2 == 0) ? ia : ib;
        conv_block(c, "rm.int" + std::to_string(i) + "." + std::to_string(b), in, ldi, H, W, ci, top, out, top, s,
                   B, hl(LEVELS));
        in = out;
        ci = top;
        ldi = top;
      }
    x = in;
    ldx = top;
  }
  // decoder
  int C = top;
  for (int i = 0; i < LEVELS; ++i) {
    const int co = C / 2;
    const std::string q = "rm.dec" + std::to_string(i);
    float* cb = catb[LEVELS - 1 - i];
    {
      ConvArgs a;
      a.x = x;
      a.ldx = ldx;
      a.T_in = H;
      a.W_in = W;
      a.C_in = C;
      a.w = c.W(q + ".up.w");
      a.ldw = C;
      a.w_ts = (long long)4 * co * C;
      a.taps = 4;
      a.KH = 2;
      a.KW = 2;
      a.y = cb;
      a.ldy = 2 * co;
      a.T_out = H;
      a.W_out = W;
      a.N = 4 * co;
      a.out_map = OUT_UPSAMPLE2D;
      a.out_cv = co;
      a.bias = c.W(q + ".up.b");
      a.act = ACT_RELU;
      a.batch = B;
      a.x_bs = (long long)H * W * ldx;
      a.y_bs = (long long)(2 * H) * (2 * W) * 2 * co;
      a.h_in = hl(LEVELS - i);  // the tap at h + 1 reads zero at an image's own last row
      run2(c, a, s, 2.0 * B * H * W * (double)C * co * 9);
    }
    H *= 2;
    W *= 2;
    float* da = c.buf<float>("rm.da", (size_t)B * Fc * NMEL * C_BASE, s);
    float* db = c.buf<float>("rm.db", (size_t)B * Fc * NMEL * C_BASE, s);
    const float* in = cb;
    int ci = 2 * co, ldi = 2 * co;
    for (int b = 0; b < NBLK; ++b) {
      float* out = (b % 2 == 0) ? da : db;
      conv_block(c, q + "." + std::to_string(b), in, ldi, H, W, ci, co, out, co, s, B, hl(LEVELS - 1 - i));
      in = out;
      ci = co;
      ldi = co;
    }
    x = in;
    ldx = co;
    C = co;
  }
  // cnn (16 -> 3, 3x3, bias) -> [Fc][3*128] (index c*128 + w) -> BiGRU -> Linear + sigmoid
  float* cn = c.buf<float>("rm.cnn", (size_t)B * Fc * NMEL * 3, s);
  run2(c, c2d(x, ldx, H, W, C_BASE, c.W("rm.cnn.w"), 3, c.W("rm.cnn.b"), cn, 3, B, hl(0)), s);
  float* feat = c.buf<float>("rm.feat", (size_t)B * Fc * 3 * NMEL, s);
  check(nhwc_to_hcw(cn, B * Fc, NMEL, 3, feat, s), "nhwc_to_hcw");
  float* gi = c.buf<float>("rm.gi", (size_t)B * Fc * 6 * GRU_H, s);
  run1(c, lin(feat, 3 * NMEL, B * Fc, 3 * NMEL, c.W("rm.gru.wih"), 6 * GRU_H, c.W("rm.gru.bih"), gi, 6 * GRU_H), s);
  float* go = c.buf<float>("rm.gruout", (size_t)B * Fc * 2 * GRU_H, s);
  gru_bidir_run(c, gi, B, Fc, c.W("rm.gru.whh_f"), c.W("rm.gru.bhh_f"), c.W("rm.gru.whh_b"), c.W("rm.gru.bhh_b"), go, -1,
                s, hl(0), beside_gru);
  ConvArgs f = lin(go, 2 * GRU_H, B * Fc, 2 * GRU_H, c.W("rm.fc.w"), NCLS, c.W("rm.fc.b"), sal, NCLS);
  f.act = ACT_SIGMOID;
  run1(c, f, s);
}

// The one RMVPE pass: mel -> frame padding -> bn0 -> E2E, 64 images at a time -> salience copy -> decode, on the B rows
// `r` describes (row b at audio + b*lda). f0 row b lands at f0 + b*ldf and its salience (optional) at
// hidden + b*ld_hidden*360. rmvpe_forward, _b and _v (runtime.h) are its entries.
// nv == nullptr: B rows of r.n_max samples; frames past mel2hidden's 32000-frame chunk (RMVPE.py:459-481) run by chunk.
// nv[B] (host): row b has nv[b] <= r.n_max samples, F_b = 1 + nv[b] / 160 frames, and runs as an image of
// Fp_b = 32 ceil(F_b / 32) frames inside [B][Fp_max][128]. In every stage a row's valid values are those of this pass
// on that row alone, up to summation order:
//   - the mel reflect-pads each row at its own end (samples past nv[b] are never read); the STFT and mel GEMMs run over
//     all B F_max frames, a row's frames past F_b on the zeros after it (finite, never read);
//   - the frame padding reflects about each row's own F_b up to Fp_b, zeros after;
//   - the U-Net and the BiGRU take the rows' heights (e2e_chunk);
//   - the decode and the salience copy stop at F_b.
// The 32000-frame chunking is not taken in this form: a row that long is refused.
static int64_t rmvpe_rows(Ctx& c, const float* audio, const Rows& r, const int64_t* nv, int64_t lda, float thred,
                          double* f0, int64_t ldf, float* hidden, int64_t ld_hidden, hipStream_t s, GruHook hook) {
  if (r.n_min < NFFT / 2 + 1) throw Error(RVCX_E_SHAPE, "rmvpe: input shorter than 513 samples");
  const int B = r.B;
  const int64_t n = r.n_max, F64 = 1 + n / HOP;
  if (F64 > ldf) throw Error(RVCX_E_CAPACITY, "rmvpe: output needs " + std::to_string(F64) + " frames per row");
  if (hidden && F64 > ld_hidden)
    throw Error(RVCX_E_CAPACITY, "rmvpe: salience needs " + std::to_string(F64) + " frames per row");
  const int chunk = 32000;
  if (nv && 32 * ((F64 - 1) / 32 + 1) > chunk)
    throw Error(RVCX_E_SHAPE, "rmvpe: a row of more than 32000 padded frames takes the single-row call");
  const int F = (int)F64, Fp = 32 * ((F - 1) / 32 + 1);
  // the strides the pass itself writes: the caller's with lengths, else back to back and staged where those are wider
  const int64_t sf = nv ? ldf : F, sh = nv ? ld_hidden : F;
  const Staged<double> f0s(c, "rm.f0v", f0, ldf, sf, B, s);
  const Staged<float> hids(c, "rm.hidv", hidden, ld_hidden * NCLS, sh * NCLS, B, s);
  // per-row lengths on device: n | F | the image heights Fp >> level, level 0 .. LEVELS
  LenCols len(3 + LEVELS, nv ? B : 0);
  const int32_t *dn = nullptr, *dF = nullptr, *dH = nullptr;
  if (nv) {
    for (int b = 0; b < B; ++b) {
      const int Fb = (int)(1 + nv[b] / HOP), Fpb = 32 * ((Fb - 1) / 32 + 1);
      if (Fpb - Fb >= Fb) check(hipErrorInvalidValue, "pad_frames");  // reflect_pad_rows' refusal of that row alone
      len.at(0, b) = (int32_t)nv[b];
      len.at(1, b) = Fb;
      for (int l = 0; l <= LEVELS; ++l) len.at(2 + l, b) = Fpb >> l;
    }
    len.upload(c, "rm.lens", s);
    dn = len.col(0), dF = len.col(1), dH = len.col(2);
  }
  // MelSpectrogram (RMVPE.py:388-417): centre reflect pad 512, F frames, the mel GEMM over all B F rows at once
  float* mel = c.buf<float>("rm.melout", (size_t)B * F * NMEL, s);
  mel_forward(c, MEL, "rm.", audio, n, lda, B, MelFrames{NFFT / 2, NFFT / 2, false, F, F, false}, mel, s, dn);
  // mel2hidden (RMVPE.py:445-482): reflect-pad frames to a multiple of 32, E2E per 32000-frame chunk
  float* img = c.buf<float>("rm.img", (size_t)B * Fp * NMEL, s);
  if (nv) {
    check(reflect_pad_rows_v(mel, dF, dH, F, Fp, NMEL, img, s, B), "pad_frames");
  } else if (Fp > F) {
    check(reflect_pad_rows(mel, F, NMEL, Fp - F, img, s, B), "pad_frames");
  } else {
    RVCX_HIP(hipMemcpyAsync(img, mel, (size_t)B * F * NMEL * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  const auto& bn0 = c.host[2].at("__bn0__").v;
  check(affine_inplace(img, (long long)B * Fp * NMEL, bn0[0], bn0[1], s), "bn0");
  float* sal = c.buf<float>("rm.sal", (size_t)B * Fp * NCLS, s);
  // the first E2E pass takes the caller's hook; the later ones get none
  auto hook_once = [&] { return std::exchange(hook, nullptr); };
  if (Fp <= chunk) {
    for (int b0 = 0; b0 < B; b0 += 64) {  // the BiGRU keeps 4 co-resident workgroups per sequence
      const int nb = std::min(64, B - b0);
      e2e_chunk(c, img + (size_t)b0 * Fp * NMEL, Fp, sal + (size_t)b0 * Fp * NCLS, s, hook_once(), nb,
                dH ? dH + b0 : nullptr, B);
    }
  } else {
    // every chunk is an independent E2E pass (RMVPE.py:459-481: the U-Net pads each chunk's edges, the BiGRU
    // restarts); a sequence's full 32000-frame chunks lie back to back, so they go through as one batch (as the
    // short branch batches sequences), the shorter tail chunk as a second pass
    const int nfull = Fp / chunk, tail = Fp - nfull * chunk;
    for (int b = 0; b < B; ++b) {
      for (int k0 = 0; k0 < nfull; k0 += 8) {  // <= 8 chunks per pass: ~13 GB of U-Net activations
        const int nb = std::min(8, nfull - k0);
        const size_t r0 = (size_t)b * Fp + (size_t)k0 * chunk;
        e2e_chunk(c, img + r0 * NMEL, chunk, sal + r0 * NCLS, s, hook_once(), nb);
      }
      if (tail > 0) {
        const size_t r0 = (size_t)b * Fp + (size_t)nfull * chunk;
        e2e_chunk(c, img + r0 * NMEL, tail, sal + r0 * NCLS, s, hook_once());
      }
    }
  }
  if (hidden)
    for (int b = 0; b < B; ++b)
      RVCX_HIP(hipMemcpyAsync(hids.p + (size_t)b * sh * NCLS, sal + (size_t)b * Fp * NCLS,
                              (size_t)(nv ? len.at(1, b) : F) * NCLS * sizeof(float), hipMemcpyDeviceToDevice, s));
  check(rmvpe_decode(sal, F, NCLS, thred, f0s.p, s, B, Fp, dF, sf), "decode");
  f0s.copy_out(s);
  hids.copy_out(s);
  return F;
}

int64_t rmvpe_forward_b(Ctx& c, const float* audio, int64_t n, int64_t lda, int B, float thred, double* f0,
                        int64_t cap, float* hidden, hipStream_t s, GruHook beside_gru) {
  const int64_t ld = std::min(cap, 1 + n / HOP);  // back to back; a cap below the frame count is refused as a stride is
  return rmvpe_rows(c, audio, Rows("rmvpe", n, B, lda), nullptr, lda, thred, f0, ld, hidden, ld, s, std::move(beside_gru));
}

int64_t rmvpe_forward_v(Ctx& c, const float* audio, const int64_t* nv, int64_t lda, int B, float thred, double* f0,
                        int64_t ldf, int64_t* F_out, float* hidden, int64_t ld_hidden, hipStream_t s,
                        bool force_ragged) {
  const Rows r("rmvpe", nv, B, lda);
  const int64_t F = rmvpe_rows(c, audio, r, r.equal && !force_ragged ? nullptr : nv, lda, thred, f0, ldf, hidden,
                               ld_hidden, s, nullptr);
  if (F_out)
    for (int b = 0; b < B; ++b) F_out[b] = 1 + nv[b] / HOP;
  return F;
}

}  // namespace rvcx
