/*
 * rvcx — kernel-level entry points for the numerics tests. Exported from librvcx.so beside the public C ABI
 * (include/rvcx.h) but not part of it: a product links rvcx.h alone. Conventions as there (device pointers, the
 * call is asynchronous on `stream`, rvcx_status returned, rvcx_last_error for the message).
 */
#ifndef RVCX_TEST_H_
#define RVCX_TEST_H_

#include "rvcx.h"

#ifdef __cplusplus
extern "C" {
#endif

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
  int b_kn, lowp;                      /* weights stored [C_in][N]; the reduced-precision opt-in */
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

/* The generator's harmonic source alone, as the decoder of the loaded configuration computes it: NSF SineGen +
 * l_linear + tanh (k_sine_cum / k_sine, csrc/aux_kernels.hip) or the 9-harmonic MRF source (csrc/source_harm.hip).
 * d_f0 [B][T] -> d_har [B][T * upp]. d_eps_src as rvcx_dec_only takes it (NSF: [B][T * upp] N(0, 1); MRF:
 * [B][T * upp][9] N(0, 1) then [B][9] U(0, 1) initial phases; NULL: drawn from `seed`). RVCX_E_STATE without a
 * finalized pitch-guided synthesizer with one of these two decoders. */
int rvcx_dec_source(rvcx_ctx* ctx, int B, int T, const float* d_f0, const float* d_eps_src, uint64_t seed, float* d_har,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RVCX_TEST_H_ */
