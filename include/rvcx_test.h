/*
 * rvcx — kernel-level entry points for the numerics tests. Exported from librvcx.so beside the public C ABI
 * (include/rvcx.h) but not part of it: a product links rvcx.h alone, and nothing there refers to a declaration here.
 * Every entry that exists for the tests or for A/B timing lives in this header: the single kernels (convs, attention,
 * ResBlock pair, Performer, k-means, BiGRU, harmonic source, RefineGAN's three), the planner query and the per-context
 * switches that only comparisons use (rvcx_set_conv_math, rvcx_set_dec_window). Conventions as in rvcx.h (device
 * pointers, the call is asynchronous on `stream`, rvcx_status returned, rvcx_last_error for the message).
 */
#ifndef RVCX_TEST_H_
#define RVCX_TEST_H_

#include "rvcx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Contraction arithmetic of every convolution / linear / attention matmul of this context (replaces nothing in
 * the reference; torch's fp32 CPU conv is what every mode reproduces): 0 = default (3), 1 = fp32-input MFMA
 * (v_mfma_f32_32x32x2_f32, an exact fp32 fma chain at 157 TF), 2 = fp32 through an exact 3-way bf16 split of both
 * operands with the six significant plane products on bf16 MFMA (error below fp32's own rounding, 2.67x the
 * MFMA rate), 3 = as 2, except that the generator's weight-streamed convs and fused ResBlock pairs split both
 * operands into two fp16 planes (x = h + 2^-11 l, 11 significand bits each) with three plane products into two
 * fp32 accumulators (csrc/split_bf16.h; error against fp64 measured at or below the fp32-input MFMA's, 5.3x the
 * fp32 MFMA rate). Env RVCX_CONV_MATH=f32 | split | h16 sets the process default when RVCX_EXPERIMENTAL=1. */
int rvcx_set_conv_math(rvcx_ctx* ctx, int mode);

/* One Conv1d forward, time-major: d_x [T][C_in], d_w [taps][N][C_in] (torch weight [N][C_in][taps] permuted),
 * d_bias [N] (optional), d_y [T_out][N]; y[t] = bias + sum_k W[k] x[t*stride - pad + k*dilation] (zero outside).
 * The kernel family behind every contraction of the path, exposed for numerics tests; replaces
 * torch.nn.Conv1d.forward as used throughout rvc/lib/algorithm (e.g. residuals.py:34-80). math as
 * rvcx_set_conv_math's mode, plus 3 = the split arithmetic on the weight-streamed kernel (weights pre-split in HBM; 1-D stride-1 convs with
 * C_in % 32 == 0 and (taps - 1) * dilation <= 64, else RVCX_E_SHAPE), 4 = the split arithmetic on the gather-streamed
 * kernel (weights pre-split in HBM, A gathered per step, split-K by the size policy; C_in % 32 == 0), 5 = the
 * two-plane fp16 split on the weight-streamed kernel (rvcx_set_conv_math mode 3's generator arithmetic), 6 = its fp16
 * hi planes alone (the realtime reduced-precision mode); 5 and 6 take the shapes 3 does; 7 = the two-plane fp16 split
 * on the gather-streamed kernel (the shapes 4 takes). */
int rvcx_conv1d(rvcx_ctx* ctx, const float* d_x, int64_t T, int C_in, const float* d_w, const float* d_bias, int N,
                int taps, int dilation, int pad, int stride, int math, float* d_y, int64_t T_out, void* stream);

/* The generator's fused conv form, time-major (rvcx_conv1d's layouts, stride 1, T_out = T + 2 pad - (taps - 1)
 * dilation): y = acc(act(conv(pre(x)) + bias) + res), pre = leaky ReLU(pre_slope) when pre_act = 1 (else identity),
 * act = leaky ReLU(slope) when act = 1, res
 * optional ([T_out][N]), acc_mode 0 store, 1 y + v, 2 (y + v) / acc_div -- one ResBlock conv (residuals.py:71-80:
 * convs1 with act, convs2 with the residual and the ResBlock mean on the last pair) or one ConvTranspose phase group
 * (hifigan_nsf.py:184-199) in the two-plane fp16 split. kernel 0 = the size policy's route, 1 = the weight-streamed
 * kernel (conv_wsb.hip, the tile the policy picks), 2 = the weight-stationary kernel (conv_wst.hip: C_in = N in {64,
 * 128}, 2-3 taps, (taps - 1) dilation <= 16, else RVCX_E_SHAPE). Exposed for numerics tests; C_in % 32 == 0. */
int rvcx_conv1d_gen(rvcx_ctx* ctx, const float* d_x, int64_t T, int C_in, const float* d_w, const float* d_bias,
                    int N, int taps, int dilation, int pad, int pre_act, float pre_slope, int act, float slope,
                    const float* d_res, int acc_mode, float acc_div, int kernel, float* d_y, void* stream);

/* One 1-D contraction in any form the runtime issues (csrc/runtime_synth.cpp, runtime_fe.cpp), described field by
 * field as the dispatcher's own record (ConvArgs, csrc/conv_kernels.h) takes it. All pointers are device pointers, all
 * strides in floats; w is [taps][N][C_in] per group (rvcx_conv1d's layout), bias [N] per group.
 *   input     pre(x[b][row][c]) * pre_mask[b][row], zero outside [0, T_in); row = m stride - pad + tap dil
 *   value     v = act(alpha (acc + bias [+ res: res_mode 1])); res_mode 2: v + res, 3: res - v; acc_mode 1: y + v,
 *             2: (y + v) / acc_div; then v * mask[b][m]. act / pre_act: 0 none, 1 leaky ReLU(slope), 2 ReLU, 3 erf GELU,
 *             4 tanh, 5 sigmoid, 6 log(max(v, slope))
 *   batch     entry (b, g) of batch x batch_inner reads / writes at b *_bs + g *_bs2 (the masks and gate_g: b only)
 *   gate_h    > 0: y[m][c] = tanh(v[c] + g[c]) sigmoid(v[c + gate_h] + g[c + gate_h]), v = acc + bias, N = 2 gate_h,
 *             g = gate_g + b gate_g_bs; no other epilogue field
 *   ln_g      set: y[m] = LN(res[m] + v[m]) ln_g + ln_b over the N <= 1024 columns (res_mode 0, acc_mode 0)
 *   nz_har    set: + nz_b[c] + nz_w[c nz_stride] har[b nz_bs + (m nz_u + p) nz_stride] at column n = p nz_C + c (the
 *             fused NSF noise conv: nz_kk = 1, N = nz_u nz_C, an unsplit weight-streamed or weight-stationary launch)
 * The gate and the LayerNorm live in the split-K combine: they need a contraction of at least two 32-channel steps.
 * route 0 = the size policy as the runtime applies it to a static weight, 1 = exact fp32 MFMA, 2 = the LDS-staged bf16
 * split (a non-static weight), 3 = the weight-streamed tile the policy picks, 4 = gather-streamed, 5 =
 * weight-stationary. A forced route that does not admit the form returns RVCX_E_SHAPE before anything is launched; it
 * never runs on another kernel. no_splitk keeps the contraction in one slice. *kind_out (optional) gets the kernel
 * family that ran (rvcx_profile_kind_name's index), *ksplit_out (optional) the planned split count. The caller owns
 * every extent: nothing is checked against an allocation. Exposed for numerics tests. */
typedef struct {
  const float* x; const float* w; const float* bias; const float* res; const float* mask; const float* pre_mask;
  float* y;
  int T_in, C_in, N, taps, dil, pad, stride, T_out;
  int ldx, ldy, ldr;
  int batch;
  int64_t x_bs, y_bs, res_bs, mask_bs, pre_mask_bs;
  int batch_inner;
  int64_t x_bs2, w_bs2, y_bs2, res_bs2, bias_bs2;
  int pre_act; float pre_slope;
  int act; float slope; float alpha;
  int res_mode, acc_mode; float acc_div;
  int gate_h; const float* gate_g; int64_t gate_g_bs;
  const float* ln_g; const float* ln_b; float ln_eps;
  const float* nz_har; int64_t nz_bs;
  int nz_stride, nz_kk, nz_u, nz_C;
  const float* nz_w; const float* nz_b;
  int route, no_splitk;
} rvcx_conv_test_desc;
int rvcx_conv1d_ex(rvcx_ctx* ctx, const rvcx_conv_test_desc* desc, int* kind_out, int* ksplit_out, void* stream);

/* One 3x3 / pad-1 Conv2d forward, NHWC: d_x [H][W][C_in], d_w [9][N][C_in] (torch weight [N][C_in][3][3] permuted to
 * (kh * 3 + kw, N, C_in)), d_bias [N] (optional), d_y [H][W][N]; act 0 none, 1 ReLU. The RMVPE U-Net's conv
 * (RMVPE.py:13-57 ConvBlockRes, torch.nn.Conv2d(kernel 3, padding 1)), exposed for the numerics tests of its
 * few-channel kernels (C_in, N in {16, 32}: csrc/conv2d_small.hip) and deep levels: math 0 = the context's arithmetic
 * (the two-plane fp16 split by default), 1 = exact fp32 (v_mfma_f32_16x16x4_f32), 2 = the deep levels' windowed
 * gather-streamed kernel in the fp16 split (images at most 32 wide, C_in % 32 == 0, else RVCX_E_SHAPE). Other shapes
 * take the general 2-D path. */
int rvcx_conv2d3x3(rvcx_ctx* ctx, const float* d_x, int H, int W, int C_in, const float* d_w, const float* d_bias,
                   int N, int act, int math, float* d_y, void* stream);

/* One ConvTranspose2d(C_in, N, kernel 3, stride 2, padding 1, output_padding 1) forward, NHWC: d_x [H][W][C_in],
 * d_w [C_in][N][3][3] (the torch layout as stored), d_bias [N] (optional), d_y [2H][2W][N]; act 0 none, 1 ReLU. The
 * RMVPE U-Net decoder's up-conv (RMVPE.py ResDecoderBlock conv1, torch.nn.ConvTranspose2d), run as the pipeline runs
 * it: a 2x2-tap phase conv with 4 N virtual output columns whose epilogue scatters the phases. math 0 = the context's
 * arithmetic (the two-plane fp16 split on the gather-streamed kernel where it applies), 1 = exact fp32. Exposed for the
 * numerics tests. */
int rvcx_convtranspose2d_s2(rvcx_ctx* ctx, const float* d_x, int H, int W, int C_in, const float* d_w,
                            const float* d_bias, int N, int act, int math, float* d_y, void* stream);

/* The two entries above on B images of different heights in one launch, as the ragged RMVPE pass issues them
 * (rvcx_rmvpe_batch_v): d_x [B][H_max][W][C_in], H (host, [B]) each image's own height in [1, H_max], d_y
 * [B][H_max][W][N] (the up-conv: [B][2 H_max][2 W][N]). Image b's output rows below H[b] (the up-conv: 2 H[b]) are
 * those of the single-image entry on its first H[b] rows, up to summation order: a tap at a row from H[b] on reads
 * zero whatever d_x holds there. Its output rows from there on are unspecified. math as the single-image entries; the
 * kernel family and split are the planner's for B images of H_max rows. */
int rvcx_conv2d3x3_v(rvcx_ctx* ctx, const float* d_x, int B, const int* H, int H_max, int W, int C_in,
                     const float* d_w, const float* d_bias, int N, int act, int math, float* d_y, void* stream);
int rvcx_convtranspose2d_s2_v(rvcx_ctx* ctx, const float* d_x, int B, const int* H, int H_max, int W, int C_in,
                              const float* d_w, const float* d_bias, int N, int act, int math, float* d_y,
                              void* stream);

/* Multi-head attention core on the fused kernel (csrc/flash_attn.hip), time-major: d_qkv [B][T][3 H] (q | k | v, head
 * h at columns h dk .. of each, H = n_heads dk), d_out [B][T][H]: per head softmax(qscale q k^T + band) v + band(p)
 * rel_v, where, with d_rel_k / d_rel_v [2 window + 1][dk] (both or neither), band adds qscale q . rel_k[j - i + window]
 * to the logit of key j of query i for |j - i| <= window and band(p) is the probabilities of those keys
 * (MultiHeadAttention.attention with window_size, rvc/lib/algorithm/attentions.py:79-185), and d_mask [B][T]
 * (optional) fills the logits of masked query-key pairs with -1e4 (:106-107). Without the relative tables it is
 * HuBERT's attention (modeling_hubert.py HubertAttention: softmax((q dk^-0.5) k^T) v). dk 64 or 96, window <= 15.
 * Exposed for the numerics tests. */
int rvcx_flash_attention(rvcx_ctx* ctx, const float* d_qkv, int B, int T, int n_heads, int dk, float qscale,
                         const float* d_rel_k, const float* d_rel_v, int window, const float* d_mask, float* d_out,
                         void* stream);

/* One ResBlock dilation pair as one fused kernel (csrc/resblock_fused.hip), time-major: d_x, d_y [B][T][C] (distinct
 * buffers), d_w1 / d_w2 [k][C][C] (torch weight [C][C][k] permuted), d_b1 / d_b2 [C]:
 *     out = conv2(lrelu(conv1_d(lrelu(x), 0.1) + b1, 0.1)) + b2 + x     (zero padding; conv2 dilation 1)
 *     acc_mode 0: y = out; 1: y = y + out; 2: y = (y + out) / acc_div
 * Replaces one iteration of ResBlock.forward (rvc/lib/algorithm/residuals.py:71-80) and MRFLayer.forward
 * (generators/hifigan_mrf.py:45-50), plus the ResBlock mean of HiFiGANNSFGenerator.forward (hifigan_nsf.py:190-207)
 * on the last pair. C in {32, 64}, odd k, (k - 1) / 2 * dilation <= 30, else RVCX_E_SHAPE. cfg bits 0-3: 0 the
 * default kernels (the k = 3, 32-channel fp16 pairs on the weight-resident form), 1 the streamed-weight kernel for
 * every shape (comparisons; bit-identical results); bits 4-5 the arithmetic: 0 the exact 3-plane bf16 split, 1 the two-plane
 * fp16 split, 2 fp16 hi planes alone (the realtime reduced-precision mode). Exposed for numerics tests and A/B timing. */
int rvcx_resblock_pair(rvcx_ctx* ctx, const float* d_x, int B, int64_t T, int C, const float* d_w1, const float* d_b1,
                       const float* d_w2, const float* d_b2, int k, int dilation, int acc_mode, float acc_div, int cfg,
                       float* d_y, void* stream);

/* Performer (FAVOR+) linear attention on the kernels of csrc/performer_attn.hip, as FCPE's SelfAttention runs it
 * after its q / k / v projections (rvc/lib/predictors/FCPE.py: FastAttention.forward :439-459, softmax_kernel
 * :179-212, linear_attention :354-363): d_q, d_k, d_v [H][T][64], d_P [M][64] (projection_matrix, M <= 512) ->
 * d_out [H][T][64]. */
int rvcx_performer_attention(rvcx_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, int H, int T,
                             const float* d_P, int M, float* d_out, void* stream);

/* The same for B streams of one T in one set of launches: d_q, d_k, d_v, d_out [B][H][T][64]; every reduction over
 * time (ksum, ctx, the row maximum, the denominator) is per (stream, head). */
int rvcx_performer_attention_b(rvcx_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, int B, int H,
                               int T, const float* d_P, int M, float* d_out, void* stream);

/* The same for B streams of different lengths in those launches: stream b has T[b] <= T_max rows (host array) in its
 * slot of d_q, d_k, d_v, d_out [B][H][T_max][64]. Rows from T[b] on are neither read nor written, and stream b's rows
 * equal rvcx_performer_attention's on that stream alone bit for bit. */
int rvcx_performer_attention_v(rvcx_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, int B, int H,
                               const int32_t* T, int T_max, const float* d_P, int M, float* d_out, void* stream);

/* The FCPE network's input alone, as rvcx_fcpe forms it (rvc/lib/predictors/FCPE.py: Wav2Mel.extract_mel :790-813 over
 * STFT.get_mel :102-168): d_audio [n] fp32 at the loaded model's sampling rate -> d_mel [F][num_mels], the log-mel of
 * every band, F = n / hop + 1 frames (*frames_out; cap_frames >= F). Needs RVCX_MODEL_FCPE finalized. */
int rvcx_fcpe_mel(rvcx_ctx* ctx, const float* d_audio, int64_t n, float* d_mel, int64_t cap_frames,
                  int64_t* frames_out, void* stream);

/* The generator's output window on (non-zero, the default) or off for this context. The offline pipelines trim
 * t_pad_tgt samples per side of every chunk and the streaming hop reads only the start of the model's output; with
 * the window on, the HiFi-GAN generator runs on the kept samples' frames plus its receptive field. Every output is
 * the same bit for bit either way: the switch exists to show that, and for same-box timing comparisons.
 * RVCX_DEC_WINDOW=0 (with RVCX_EXPERIMENTAL=1) sets the default off at rvcx_create. */
int rvcx_set_dec_window(rvcx_ctx* ctx, int on);

/* The generator's one-sided receptive field in input frames for a synthesizer configuration (the margin the output
 * window keeps per cut side): *frames. Host only, no context. */
int rvcx_dec_margin_frames(const rvcx_synth_desc* d, int* frames);

/* What the conv planner (csrc/conv_dispatch.hip conv_plan) decides for one contraction: the kernel family (*kind, a
 * ConvKind as rvcx_profile_kind_name names them; the last one, "other": no family admits the form), its tile id
 * (*tile, -1: the family has one form), the split over K (*ksplit) and the weight image the family reads
 * (*wsplit_fmt: 0 three bf16 planes, 1 two fp16 planes, 2 the 3x3 small-channel image, -1 none). Host only: no
 * context, no GPU; the descriptor's pointers are read for nullness and 16-byte alignment alone and its `route` is not
 * read. form: the fields of the dispatcher's record a 1-D descriptor lacks (NULL = a plain 1-D form; for a 2-D
 * contraction T_in / T_out are the image heights). static_weight: the weight is a constant tensor (the streamed
 * kernels take only those). math: the context's arithmetic (rvcx_set_conv_math; 0 the default, 3 the fp16 split).
 * plan_T: the rows the launch is planned for (0 = T_out). force_kind / force_tile: a forced family / tile, -1 the
 * size policy's. */
typedef struct rvcx_conv_plan_form {
  int W_in, W_out, KH, KW, padh, padw; /* 2-D geometry (taps = KH * KW) */
  int out_map, out_cv;                 /* 1: the 2x2-phase ConvTranspose2d scatter with out_cv real channels */
  int lowp;                            /* the reduced-precision opt-in */
  int ldw;                             /* weight row stride, 0 = C_in */
  int64_t w_ts, w_bs, bias_bs;         /* weight tap stride (0 = N * C_in), per-batch weight and bias strides */
} rvcx_conv_plan_form;
int rvcx_conv_plan(const rvcx_conv_test_desc* d, const rvcx_conv_plan_form* form, int two_d, int static_weight, int math,
                   int plan_T, int force_kind, int force_tile, int* kind, int* tile, int* ksplit, int* wsplit_fmt);

/* One nearest-centroid pass of the index build (csrc/kmeans.hip k_kmeans_assign; faiss IndexFlatL2::search with
 * k = 1 inside Clustering::train): d_x [n][d], d_cent [nlist][d] fp32 -> d_assign [n] = argmin_l |x - c_l|^2, ties to
 * the lowest l; d_dist [n] (optional) the squared distance to it. d % 32 == 0 and d <= 1024, else RVCX_E_SHAPE. */
int rvcx_kmeans_assign(rvcx_ctx* ctx, const float* d_x, int64_t n, int d, const float* d_cent, int64_t nlist,
                       int32_t* d_assign, float* d_dist, void* stream);

/* One centroid update of the index build (k_kmeans_update after the stable counting sort): d_cent [nlist][d]
 * (in-out) row l becomes the mean of the rows with d_assign == l (fp64 accumulation in ascending row order, one
 * rounding); a list without rows keeps its centroid. d_sizes [nlist] (optional) = the list sizes. A row whose
 * assignment is outside [0, nlist) belongs to no list and is left out. */
int rvcx_kmeans_update(rvcx_ctx* ctx, const float* d_x, int64_t n, int d, const int32_t* d_assign, int64_t nlist,
                       float* d_cent, int64_t* d_sizes, void* stream);

/* The model rows of the group's last hop, [B_act][frames * upp] (the active streams in slot order), copied to d_dst
 * (rows ld >= frames * upp apart): gated = 0 the rows as the noise gate read them (after the clip and the volume
 * envelope), gated = 1 as the * sqrt(vol) / resample / SOLA stage read them (the gate's output; the same rows on a hop
 * where no stream cleans). Valid until the context's next compute call. RVCX_E_STATE before the first hop. */
int rvcx_rt_model_rows(rvcx_ctx* ctx, rvcx_rt* rt, int gated, float* d_dst, int64_t ld, void* stream);

/* RMVPE's BiGRU recurrence alone (csrc/gru.hip k_gru_bidir_g; nn.GRU(384, 256, bidirectional), ATen cell order), given
 * the input projections: d_gi [B][T][1536] (x W_ih^T + b_ih; forward r, z, n then backward r, z, n), W_hh [768][256]
 * and b_hh [768] per direction -> d_out [B][T][512] (forward h then backward h per step). It runs the launches RMVPE
 * runs: the context's hand-off buffer, 16 sequences per launch, one tag counter per 16-sequence slice. tag_start < 0:
 * the counters run on from the earlier launches on the buffer; tag_start >= 0 (< 2^32): the buffer is zeroed and every
 * slice's counter set to tag_start before the launch (0: a freshly zeroed buffer; a counter that T + 1 more tags would
 * carry past 2^32 zeroes the slice and restarts at 1). Any B >= 1; 1 <= T <= 2^20 (32-bit row offsets in the kernel);
 * the W_hh pointers 16-byte aligned; else RVCX_E_INVALID. */
int rvcx_gru_bidir(rvcx_ctx* ctx, const float* d_gi, int B, int T, const float* d_whh_f, const float* d_bhh_f,
                   const float* d_whh_b, const float* d_bhh_b, float* d_out, int64_t tag_start, void* stream);

/* rvcx_gru_bidir for sequences of different lengths in the same launches: T (host, [B]) each sequence's step count
 * (>= 1), d_gi [B][T_max][1536] and d_out [B][T_max][512] with T_max the longest. Sequence b's first T[b] output rows
 * are rvcx_gru_bidir's on that sequence alone with T = T[b], bit for bit (the same arithmetic in the same order; its
 * reverse direction starts at row T[b] - 1); its rows from T[b] on are not written. Every slice's tag counter advances
 * by T_max + 1. */
int rvcx_gru_bidir_v(rvcx_ctx* ctx, const float* d_gi, int B, const int* T, const float* d_whh_f, const float* d_bhh_f,
                     const float* d_whh_b, const float* d_bhh_b, float* d_out, int64_t tag_start, void* stream);

/* The generator's harmonic source alone, as the decoder of the loaded configuration computes it: NSF SineGen +
 * l_linear + tanh (k_sine_cum / k_sine, csrc/nsf_source.hip) or the 9-harmonic MRF source (csrc/source_harm.hip).
 * d_f0 [B][T] -> d_har [B][T * upp]. d_eps_src as rvcx_dec_only takes it (NSF: [B][T * upp] N(0, 1); MRF:
 * [B][T * upp][9] N(0, 1) then [B][9] U(0, 1) initial phases; NULL: drawn from `seed`). RVCX_E_STATE without a
 * finalized pitch-guided synthesizer with one of these two decoders. */
int rvcx_dec_source(rvcx_ctx* ctx, int B, int T, const float* d_f0, const float* d_eps_src, uint64_t seed, float* d_har,
                    void* stream);

/* The three elementwise kernels of the RefineGAN decoder alone (csrc/refinegan.hip), time-major rows as the decoder
 * holds them. Extents are checked before anything is launched: a null pointer or a count below 1 is RVCX_E_INVALID, a
 * geometry the kernel does not serve RVCX_E_SHAPE.
 *
 * rvcx_rg_resample_dw: torchaudio's kaiser-sinc resample(orig -> 1) on given taps (refinegan.py:410-419):
 *   y[b][t][c] = sum_k x[b][t orig + k - width][c] ker[k], zero outside [0, T_in); d_x [B][T_in][C], d_ker [K],
 *   K = 2 width + orig <= 8192 (the taps sit in LDS), d_y [B][T_out][C], 1 <= T_out <= ceil(T_in / orig). */
int rvcx_rg_resample_dw(rvcx_ctx* ctx, const float* d_x, int B, int T_in, int C, const float* d_ker, int orig, int width,
                        float* d_y, int T_out, void* stream);

/* rvcx_rg_lerp_up_cat: y[b][t][0:C] = nn.Upsample(scale_factor = rate, mode "linear")(leaky ReLU(x, slope)) at t,
 * y[b][t][C:C + Cd] = skip[b][t] (refinegan.py:426-429): d_x [B][T] rows of ldx >= C floats, d_skip [B][T rate][Cd],
 * d_y [B][T rate] rows of ldy >= C + Cd floats (columns from C + Cd on are not written). */
int rvcx_rg_lerp_up_cat(rvcx_ctx* ctx, const float* d_x, int B, int T, int C, int ldx, int rate, float slope,
                        const float* d_skip, int Cd, float* d_y, int ldy, void* stream);

/* rvcx_rg_adain: v = leaky ReLU(x + eps w[c], slope) (AdaIN, refinegan.py:74-94): d_x, d_y [B][T][C], d_w [C], d_eps
 * in the reference's layout [B][C][T] (NULL: N(0, 1) drawn from `seed` at the same index); mode 0: y = v, 1: y += v,
 * 2: y = (y + v) / div (div != 0). */
int rvcx_rg_adain(rvcx_ctx* ctx, const float* d_x, int B, int T, int C, const float* d_w, const float* d_eps,
                  uint64_t seed, float slope, float* d_y, int mode, float div, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RVCX_TEST_H_ */
