/*
 * rvcx — MI355X-native RVC v2 inference engine: public C ABI.
 *
 * Plain pointers and sizes only. All d_* pointers are device (HBM) pointers owned by the
 * caller (e.g. torch tensors' data_ptr()); every compute call is asynchronous on the given
 * hipStream_t (passed as void*; NULL = the null stream). The context owns the uploaded
 * weights, the workspace and the RNG state; one context = one device, one host thread at a
 * time. Every function returns an rvcx_status (0 = ok, < 0 = error); the message of the
 * last error is rvcx_last_error(ctx). Nothing prints and continues.
 *
 * The reference (Acelogic/Retrieval-based-Voice-Conversion-MLX) has no native code on this
 * path; each entry point below replaces a Python-level interface of the reference, cited
 * file:line (paths relative to the reference root).
 */
#ifndef RVCX_H_
#define RVCX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rvcx_ctx rvcx_ctx;

typedef enum {
  RVCX_OK = 0,
  RVCX_E_INVALID = -1, /* bad argument (null pointer, negative size, unknown name) */
  RVCX_E_SHAPE = -2,   /* tensor shape / length does not match the model */
  RVCX_E_HIP = -3,     /* HIP runtime error or kernel launch failure */
  RVCX_E_OOM = -4,     /* device allocation failed */
  RVCX_E_STATE = -5,   /* model not finalized / weights missing */
  RVCX_E_CAPACITY = -6 /* caller's output buffer too small */
} rvcx_status;

typedef enum {
  RVCX_MODEL_SYNTH = 0,
  RVCX_MODEL_HUBERT = 1,
  RVCX_MODEL_RMVPE = 2,
  RVCX_MODEL_CREPE = 3,
  RVCX_MODEL_FCPE = 4
} rvcx_model;

/* Synthesizer hyper-parameters = the 18-element ``cpt["config"]`` list of an RVC .pth
 * (rvc/train/process/extract_model.py:62-81) plus text_enc_hidden_dim (768 for v2). */
typedef struct {
  int inter_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size;
  int n_resblocks;                  /* len(resblock_kernel_sizes) (3) */
  int resblock_kernel_sizes[4];
  int resblock_dilation_sizes[4][4];
  int n_dilations;                  /* len of each dilation list (3) */
  int n_upsample;                   /* len(upsample_rates) (4) */
  int upsample_rates[8];
  int upsample_initial_channel;
  int upsample_kernel_sizes[8];
  int spk_embed_dim, gin_channels, sr, text_enc_hidden_dim;
  int no_f0;   /* 1: model without pitch guidance (cpt["f0"] == 0): TextEncoder without emb_pitch and the plain
                  HiFiGANGenerator (synthesizers.py:84, :122-139, :233-239; generators/hifigan.py:9-104) */
  int vocoder; /* decoder of a pitch-guided model (cpt["vocoder"], infer.py:478): 0 "HiFi-GAN" (NSF),
                  1 "MRF HiFi-GAN", 2 "RefineGAN" (synthesizers.py:86-118) */
} rvcx_synth_desc;

/* Create a context on HIP device `device`. */
int rvcx_create(rvcx_ctx** out, int device);
int rvcx_destroy(rvcx_ctx* ctx);
const char* rvcx_last_error(const rvcx_ctx* ctx);

/* Model structure (replaces Synthesizer(*cpt["config"]) in rvc/infer/infer.py:467-488 and
 * the hard-coded defaults of rvc_mlx/infer/infer_mlx.py:130-244). */
int rvcx_set_synth_config(rvcx_ctx* ctx, const rvcx_synth_desc* desc);

/* Weight ingestion: one fp32 host tensor in the REFERENCE layout under its REFERENCE
 * state-dict name (weight-norm already fused to ``.weight``; BatchNorm as its 4 tensors).
 * Replaces load_state_dict in rvc/infer/infer.py:480-486 (synth), HubertModel
 * from_pretrained in rvc/lib/utils.py:125-153 (hubert), RMVPE0Predictor.__init__
 * torch.load in rvc/lib/predictors/RMVPE.py:429-434 (rmvpe). */
int rvcx_upload(rvcx_ctx* ctx, int model, const char* name, const float* host, const int64_t* shape, int ndim);
/* Validate names/shapes, fold BatchNorm, repack to kernel layouts, copy to HBM. */
int rvcx_finalize(rvcx_ctx* ctx, int model);

/* HuBERT/ContentVec: hubert_model(audio[1,N])["last_hidden_state"] -> [L][768] (v2) or final_proj
 * [L][256] (v1). Replaces transformers HubertModel.forward as called at rvc/infer/pipeline.py:331-334
 * and rvc_mlx/lib/mlx/hubert.py:174-201 (pipeline_mlx.py:172-173). */
int rvcx_hubert(rvcx_ctx* ctx, const float* d_audio, int64_t n, int version, float* d_feats, int64_t cap_rows,
                int64_t* rows_out, void* stream);

/* RMVPE: RMVPE0Predictor.infer_from_audio(audio, thred) -> f0 (fp64, [F], F = 1 + n/160).
 * Replaces rvc/lib/predictors/RMVPE.py:497-513 and rvc_mlx/lib/mlx/rmvpe.py:408-412.
 * d_hidden (optional, [F][360] fp32) receives the salience (mel2hidden output). */
int rvcx_rmvpe(rvcx_ctx* ctx, const float* d_audio, int64_t n, float thred, double* d_f0, int64_t cap_frames,
               int64_t* frames_out, float* d_hidden, void* stream);

/* Batched forms over B equal-length inputs (rows of stride lda floats; HuBERT needs lda % 5 == 0 when B > 1):
 * feats [B][L][D] and f0 [B][F] (d_hidden [B][F][360]) back to back. Used by the streaming path (B streams
 * per hop) and the batched offline mode; each sequence's result equals the unbatched call's. */
int rvcx_hubert_batch(rvcx_ctx* ctx, const float* d_audio, int64_t n, int64_t lda, int B, int version, float* d_feats,
                      int64_t cap_rows, int64_t* rows_out, void* stream);
int rvcx_rmvpe_batch(rvcx_ctx* ctx, const float* d_audio, int64_t n, int64_t lda, int B, float thred, double* d_f0,
                     int64_t cap_frames, int64_t* frames_out, float* d_hidden, void* stream);

/* HuBERT over B inputs of different lengths in one launch set: row b has n[b] samples (host array) at
 * d_audio + b*lda (lda >= every n[b]; samples past n[b] are never read). Row b's features [L_b][D], L_b =
 * frames of n[b] as rvcx_hubert counts them (written to L_out[b], host, optional), land at d_feats + b*ld_rows*D;
 * ld_rows must hold the longest row's frames. The rows of a block past L_b, up to the longest row's count, are
 * overwritten with unspecified finite values. Every valid frame equals rvcx_hubert's on that input alone up to
 * summation order: the GroupNorm statistics are over the row's own frames, the positional conv sees zeros past
 * its end and attention masks its pad keys. Equal lengths take rvcx_hubert_batch's path. A row too short for
 * one frame (n[b] < 400) fails with RVCX_E_SHAPE. */
int rvcx_hubert_batch_v(rvcx_ctx* ctx, const float* d_audio, const int64_t* n, int64_t lda, int B, int version,
                        float* d_feats, int64_t ld_rows, int64_t* L_out, void* stream);

/* RMVPE over B inputs of different lengths in one launch set: row b has n[b] samples (host array) at
 * d_audio + b*lda (lda >= every n[b]; samples past n[b] are never read). Row b's f0 [F_b] fp64, F_b = 1 + n[b]/160
 * (written to F_out[b], host, optional), lands at d_f0 + b*ldf, and its salience [F_b][360] (d_hidden, optional) at
 * d_hidden + b*ld_hidden_frames*360; ldf (and ld_hidden_frames) must hold the longest row's frames, else
 * RVCX_E_CAPACITY. Values of a row past F_b are not written. Every row equals rvcx_rmvpe's on that input alone up to
 * summation order: the mel and the frame padding reflect about the row's own end, every 3x3 conv and up-conv of the
 * U-Net reads zero past the row's own last padded frame, and the BiGRU's reverse pass starts there. Equal lengths
 * take rvcx_rmvpe_batch's path, bit for bit, whatever their length (that path splits rows of more than 32000 padded
 * frames, the reference's chunk of 320 s, as rvcx_rmvpe does). Among rows of different lengths a row of more than
 * 32000 padded frames fails with RVCX_E_SHAPE: the ragged pass does not chunk. A row shorter than 513 samples fails
 * with RVCX_E_SHAPE; any other row rvcx_rmvpe refuses fails with that call's status. */
int rvcx_rmvpe_batch_v(rvcx_ctx* ctx, const float* d_audio, const int64_t* n, int64_t lda, int B, float thred,
                       double* d_f0, int64_t ldf, int64_t* F_out, float* d_hidden, int64_t ld_hidden_frames,
                       void* stream);

/* CREPE (f0 methods "crepe" / "crepe-tiny"): CREPE.get_f0(audio, f0_min, f0_max, threshold) of
 * rvc_mlx/lib/mlx/crepe.py:282-325 (the torchcrepe network of rvc/lib/predictors/f0.py:25-57; MLX dispatch
 * rvc_mlx/lib/mlx/pitch_extractors.py:155-156). Weights: RVCX_MODEL_CREPE under torchcrepe's names (conv1..6 +
 * _BN, classifier), full or tiny by conv1's filter count. d_audio [n] fp32 @16 kHz (n > 512) -> d_f0 [F] fp32,
 * F = 1 + n/160; d_periodicity ([F], filtered) and d_probs ([F][360], the sigmoid outputs) are optional. */
int rvcx_crepe(rvcx_ctx* ctx, const float* d_audio, int64_t n, float f0_min, float f0_max, float threshold,
               float* d_f0, float* d_periodicity, float* d_probs, int64_t cap_frames, int64_t* frames_out,
               void* stream);

/* rvcx_crepe with a choice of semantics: 0 = as rvcx_crepe (the MLX port's CREPE.get_f0); 1 = rvc/'s CREPE.get_f0
 * (rvc/lib/predictors/f0.py:31-55): torchcrepe.predict's framing (zero padding of 512, unbiased std), its default
 * viterbi decoder (torchcrepe.decode.viterbi: the sigmoid outputs outside [f0_min, f0_max] masked, softmax over the
 * bins, librosa.sequence.viterbi with the +-11-bin triangular transition matrix), periodicity = the output at the
 * decoded bin, then torchcrepe.filter.median(periodicity, 3), filter.mean(f0, 3) and f0 = 0 where the periodicity <
 * threshold. torchcrepe dithers the decoded cents with scipy.stats.triang noise on [-20, 20] cents: d_dither [F]
 * (optional, semantics 1 only) supplies it, NULL decodes without. torchcrepe / librosa are not importable here: the
 * restatement follows their published source (parity unpinned; tests/test_gpu_crepe.py checks it against
 * oracle/crepe.py's numpy restatement). Any n > 0. In rvcx_pipeline_opts: f0_method 2 (no dither). */
int rvcx_crepe_ex(rvcx_ctx* ctx, const float* d_audio, int64_t n, float f0_min, float f0_max, float threshold,
                  int semantics, const float* d_dither, float* d_f0, float* d_periodicity, float* d_probs,
                  int64_t cap_frames, int64_t* frames_out, void* stream);
/* The decode alone (the tail of rvcx_crepe_ex after the network: CREPE._decode + filters for semantics 0,
 * torchcrepe's viterbi + rvc/'s filters for 1) on caller-given probabilities d_probs [F][360]. */
int rvcx_crepe_decode(rvcx_ctx* ctx, const float* d_probs, int64_t F, float f0_min, float f0_max, float threshold,
                      int semantics, const float* d_dither, float* d_f0, float* d_periodicity, void* stream);

/* FCPE (f0 method "fcpe" of rvc/): the network of rvc/lib/predictors/FCPE.py, as FCPEInfer builds it from a
 * checkpoint {"config": ..., "model": state_dict} (:731-756). rvcx_fcpe_desc carries the sizes of that config
 * (config["mel"]: sampling_rate, n_fft, win_size, hop_size, num_mels, fmin, fmax -- Wav2Mel / STFT :767-783, :79-100;
 * config["model"]: n_layers, n_chans, out_dims -- FCPE.__init__ :571-647; the attention is SelfAttention's 8 heads
 * x 64 with nb_features = projection_matrix.shape[0], :462-512). Set it before rvcx_finalize(RVCX_MODEL_FCPE).
 * Weights: RVCX_MODEL_FCPE under the module's state-dict names (stack.*, decoder._layers.N.{norm, attn.to_q/k/v/out,
 * attn.fast_attention.projection_matrix, conformer.net.{0,2,4.conv,6}}, norm, dense_out with its weight-norm fused
 * to dense_out.weight, cent_table). Supported: n_fft == win_size, win_size % 32 == hop_size % 32 == 0, num_mels % 32
 * == 0, n_chans % 32 == 0 and <= 1024, nb_features <= 512, else RVCX_E_SHAPE. */
typedef struct {
  int sampling_rate, n_fft, win_size, hop_size, num_mels;
  float fmin, fmax;
  int n_layers, n_chans, out_dims;
} rvcx_fcpe_desc;
int rvcx_set_fcpe_config(rvcx_ctx* ctx, const rvcx_fcpe_desc* desc);

/* FCPEInfer.__call__(audio, sr = sampling_rate, threshold) (FCPE.py:758-764) and, with interp_uv,
 * FCPEF0Predictor.compute_f0's tail (:904-910). d_audio [n] fp32 at the config's sampling rate (no resampling:
 * Wav2Mel.extract_mel's sample_rate == self.sample_rate branch, :790-813) -> mel (STFT.get_mel :102-168: pad
 * (win - hop) / 2 left and max((win - hop + 1) / 2, win - n - left) right, reflect when that is < n else zeros;
 * |STFT|, center = False; log mel; F = n / hop + 1 frames, the last one repeated when the STFT gives one fewer) ->
 * FCPE.forward (:657-665: conv stack, n_layers x (Performer attention + Conformer conv module), LayerNorm, dense_out,
 * sigmoid) -> salience [F][out_dims] -> decoder_mode 0 cents_local_decoder (:696-711, the default "local_argmax") or
 * 1 cents_decoder (:683-694, "argmax"), cent_to_f0 (:713-714); f0 = 0 where the frame maximum <= threshold.
 * interp_uv = 1: FCPEF0Predictor.post_process (:877-902) follows: the track is expanded to pad_to frames
 * (repeat_expand, nearest; pad_to <= 0: F) and interpolated linearly through the unvoiced frames, the first / last
 * voiced value held at the ends, zeros when no frame is voiced (:908-909).
 * d_f0: fp64 [max(F, pad_to)] (the raw track holds the network's fp32 values exactly; np.interp's output is fp64);
 * d_salience (optional) fp32 [F][out_dims]. cap_frames >= the frames written, *frames_out = their count. */
int rvcx_fcpe(rvcx_ctx* ctx, const float* d_audio, int64_t n, float threshold, int decoder_mode, int interp_uv,
              int64_t pad_to, double* d_f0, float* d_salience, int64_t cap_frames, int64_t* frames_out, void* stream);
/* rvcx_fcpe's raw track for B streams of n samples each in one batched forward (one set of launches per layer for
 * all streams, not a loop): row b at d_audio + b * ld (ld >= n). Per row the semantics of rvcx_fcpe with interp_uv = 0:
 * F = n / hop + 1 frames, f0 = 0 where the frame maximum <= threshold. Everything the network pads or reduces over
 * time (the mel's reflect / zero padding and repeated last frame, the convs' zero padding, the GroupNorm statistics,
 * the attention's sums) is each stream's own. d_f0: fp64 [B][F]; d_salience (optional) fp32 [B][F][out_dims]. The
 * interp_uv / pad_to tail stays with rvcx_fcpe. */
int rvcx_fcpe_b(rvcx_ctx* ctx, const float* d_audio, int64_t n, int64_t ld, int B, float threshold, int decoder_mode,
                double* d_f0, float* d_salience, void* stream);
/* rvcx_fcpe's raw track over B inputs of different lengths in one launch set: row b has n[b] samples (host array) at
 * d_audio + b*lda (lda >= every n[b]; samples past n[b] are never read). Row b's f0 [F_b] fp64, F_b = n[b]/hop + 1
 * (written to F_out[b], host, optional), lands at d_f0 + b*ldf, and its salience [F_b][out_dims] (d_salience,
 * optional) at d_salience + b*ld_sal_frames*out_dims; ldf (and ld_sal_frames) must hold the longest row's frames, else
 * RVCX_E_CAPACITY. Values of a row past F_b are not written. Every row equals rvcx_fcpe's (interp_uv = 0) on that input
 * alone up to summation order: the mel reflects about the row's own end and repeats the row's own last frame, the
 * k = 3 convs and the depthwise conv read zero past the row's own last frame, the GroupNorm statistics and the
 * attention's sums run over the row's own frames. Equal lengths take rvcx_fcpe_b's path and B = 1 rvcx_fcpe's, bit
 * for bit. Among rows of different lengths a row short enough for the mel's zero padding (n <= (win - hop + 1)/2: 432 samples
 * for win 1024, hop 160) fails with RVCX_E_SHAPE: the per-row front end reflects. B < 1 is
 * RVCX_E_INVALID. The interp_uv / pad_to tail stays with rvcx_fcpe. */
int rvcx_fcpe_batch_v(rvcx_ctx* ctx, const float* d_audio, const int64_t* n, int64_t lda, int B, float threshold,
                      int decoder_mode, double* d_f0, int64_t ldf, int64_t* F_out, float* d_salience,
                      int64_t ld_sal_frames, void* stream);
/* The decode alone (the tail of rvcx_fcpe after the network: FCPE.py:683-714, :877-902) on caller-given salience
 * d_salience [F][out_dims], with the loaded model's cent table and hop / sampling rate. d_f0 fp64 [pad_to when
 * interp_uv and pad_to > 0, else F]. */
int rvcx_fcpe_decode(rvcx_ctx* ctx, const float* d_salience, int64_t F, float threshold, int decoder_mode,
                     int interp_uv, int64_t pad_to, double* d_f0, void* stream);

/* split_audio.process_audio (rvc/lib/tools/split_audio.py:5-27; rvc/infer/infer.py:282-284): the non-silent
 * intervals librosa.effects.split(audio, top_db=-silence_thresh_db, frame_length=int(min_silence_len_ms/1000*sr),
 * hop_length=frame_length//2) returns. d_audio [n] fp64 on device; intervals (HOST [cap][2] int64, start/end
 * samples) receives *count of them; the call synchronises the stream (the edges are host logic over the frame
 * RMS computed on device). RVCX_E_CAPACITY when more than cap intervals. */
int rvcx_split_audio(rvcx_ctx* ctx, const double* d_audio, int64_t n, int sr, double silence_thresh_db,
                     int min_silence_len_ms, int64_t* intervals, int64_t cap, int64_t* count, void* stream);

/* RMVPE0Predictor.decode (rvc/lib/predictors/RMVPE.py:515-540; rvc_mlx/lib/mlx/rmvpe.py:357-406):
 * salience [F][360] fp32 -> f0 [F] fp64 (argmax, +-4-bin weighted cents, threshold, 10 * 2^(c/1200), 10 -> 0). */
int rvcx_rmvpe_decode(rvcx_ctx* ctx, const float* d_hidden, int64_t F, float thred, double* d_f0, void* stream);

/* f0 post-processing of Pipeline.get_f0 (rvc/infer/pipeline.py:278-291): f0 *= 2^(semitones/12),
 * mel quantisation to coarse 1..255. Writes coarse (int32), pitchf (fp32) and shifted f0 (fp64, optional). */
int rvcx_f0_post(rvcx_ctx* ctx, const double* d_f0, int64_t F, double semitones, int32_t* d_coarse, float* d_pitchf,
                 double* d_f0_shifted, void* stream);

/* Autotune.autotune_f0 in place (rvc/infer/pipeline.py:151-162; rvc_mlx/infer/pipeline_mlx.py:72-80):
 * f0 += (nearest note - f0) * strength. skip_unvoiced = 1 leaves f0 <= 0 frames untouched (MLX). */
int rvcx_f0_autotune(rvcx_ctx* ctx, double* d_f0, int64_t F, double strength, int skip_unvoiced, void* stream);

/* Synthesizer.infer (rvc/lib/algorithm/synthesizers.py:206-243; rvc_mlx/lib/mlx/synthesizers.py:193-235).
 * For a model without pitch guidance (no_f0) d_pitch / d_pitchf may be NULL and are ignored (:233-239); the
 * same holds for d_f0 of rvcx_dec_only and d_pitch / d_pitchf of rvcx_voice_conversion.
 * phone [B][T][E], lengths [B], pitch [B][T], pitchf [B][T], sid [B] -> out [B][T*upp].
 * Source noise layout by decoder: HiFi-GAN (NSF) [B][T*upp] (randn_like, generators/hifigan.py:223); MRF HiFi-GAN
 * [B][T*upp][9] (randn_like(sine_waves), hifigan_mrf.py:222) followed by the [B][9] initial phases (torch.rand,
 * :174-178, element 0 of each row unused); RefineGAN [B][T*upp] (randn_like, refinegan.py:233) then [B][1]
 * (torch.rand, :203) then, per upsampling stage and ParallelResBlock branch j = 0..2, the AdaIN draws (in, out)
 * [B][C_stage][T_stage] each (refinegan.py:90); no source for models without pitch guidance.
 * d_eps_z ([B][I][T], reference layout of randn_like(m_p)) and d_eps_src ([B][T*upp], randn_like at
 * generators/hifigan.py:223) are optional injected noise; when NULL the noise is drawn from the
 * context's Philox stream keyed by `seed`. d_zp / d_z (optional, [B][T][I]) receive z_p and z. */
int rvcx_synth_infer(rvcx_ctx* ctx, int B, int T, const float* d_phone, const int32_t* d_lengths,
                     const int32_t* d_pitch, const float* d_pitchf, const int32_t* d_sid, const float* d_eps_z,
                     const float* d_eps_src, uint64_t seed, float* d_out, float* d_zp, float* d_z, void* stream);
/* Synthesizer.infer with its remaining arguments and full return value (synthesizers.py:206-243): rate (the partial
 * re-synthesis of :230-234; < 0 = None) keeps z_p, x_mask and nsff0 [:, head:] before the flow with the reference's
 * head = int(T (1 - rate)) and Python's slice semantics: a negative head (rate > 1) keeps the last -head frames (all T
 * when -head >= T); a rate that keeps no frame (rate 0) is RVCX_E_SHAPE. d_out holds [B][T' upp] and d_zp / d_z
 * [B][T'][I] with T' the kept frames; *t_out = T'.
 * d_m_p / d_logs_p (optional) [B][T][I] receive the TextEncoder's m_p / logs_p (the rest of the tuple :243). Noise as
 * rvcx_synth_infer (d_eps_z over all T frames, d_eps_src over the T - head synthesized ones). */
int rvcx_synth_infer_ex(rvcx_ctx* ctx, int B, int T, const float* d_phone, const int32_t* d_lengths,
                        const int32_t* d_pitch, const float* d_pitchf, const int32_t* d_sid, double rate,
                        const float* d_eps_z, const float* d_eps_src, uint64_t seed, float* d_out, float* d_zp,
                        float* d_z, float* d_m_p, float* d_logs_p, int* t_out, void* stream);

/* HiFiGAN-NSF generator alone (config C3): dec(z, f0, g=emb_g(sid)) with z in reference layout
 * [B][I][T] (rvc/lib/algorithm/generators/hifigan_nsf.py:173-212). out [B][T*upp]. */
int rvcx_dec_only(rvcx_ctx* ctx, int B, int T, const float* d_z, const float* d_f0, const int32_t* d_sid,
                  const float* d_eps_src, uint64_t seed, float* d_out, void* stream);

/* Pipeline.voice_conversion on one padded chunk (rvc/infer/pipeline.py:293-376;
 * rvc_mlx/infer/pipeline_mlx.py:166-261): HuBERT -> [speaker-embedding retrieval from the loaded
 * feature index when index_rate > 0] -> x2 nearest upsample -> protect blend -> Synthesizer.infer,
 * all on device. d_audio [n] @16 kHz (already filtered and padded); d_pitch/d_pitchf [>= n/160].
 * Output out [p_len*upp], p_len = min(n/160, 2L). */
int rvcx_voice_conversion(rvcx_ctx* ctx, const float* d_audio, int64_t n, const int32_t* d_pitch,
                          const float* d_pitchf, int sid, float protect, double index_rate, const float* d_eps_z,
                          const float* d_eps_src, uint64_t seed, float* d_out, int64_t cap, int64_t* n_out,
                          void* stream);

/* Pipeline high-pass (rvc/infer/pipeline.py:22-27: signal.butter(5, 48, 'high', fs=16000)) as
 * transfer-function coefficients b[order+1], a[order+1] and lfilter_zi(b, a) zi[order]; used by
 * rvcx_pipeline's zero-phase filtfilt (padtype 'odd', padlen 3*(order+1)). */
int rvcx_set_highpass(rvcx_ctx* ctx, const double* b, const double* a, const double* zi, int order);

/* The same high-pass as second-order sections sos[nsec][6] = (b0 b1 b2 a0 a1 a2) per section (scipy
 * butter(5, 48, 'high', fs=16000, output='sos'): exact zpk sections). When set, filtfilt runs as a
 * chunk-parallel scan over the sections (stable: each section's 2x2 state matrix is well conditioned, unlike
 * the order-5 companion form). Call after rvcx_set_highpass (which sets the padding length). */
int rvcx_set_highpass_sos(rvcx_ctx* ctx, const double* sos, int nsec);
/* signal.filtfilt(bh, ah, audio) then np.pad(..., (t_pad, t_pad), 'reflect') (pipeline.py:439, :459):
 * d_audio [n] fp64 -> d_pad64 (optional) / d_pad32 [n + 2 t_pad]. */
int rvcx_highpass_pad(rvcx_ctx* ctx, const double* d_audio, int64_t n, int64_t t_pad, double* d_pad64, float* d_pad32,
                      void* stream);

/* scipy.signal.resample_poly's output length for n input frames: ceil(n*up/down) after gcd reduction. Host only. */
int rvcx_resample_poly_len(int64_t n, int up, int down, int64_t* n_out);

/* Decode, channel downmix and scipy.signal.resample_poly(x, up, down) (window ("kaiser", 5.0), padtype "constant")
 * in one launch: what the file loader does on the host before the pipeline, and a converted output delivered at
 * another rate after it. B rows, ragged. d_x: interleaved frames of `dtype` (0 f64, 1 f32, 2 i16 scaled by 2^-15,
 * 3 i32 scaled by 2^-31; 24-bit WAV data is left-justified int32), `channels` per frame, row stride ldx frames;
 * n[b] >= 1 frames per row (host array). The mono sample is the channels' fp64 sum in channel order / channels.
 * d_taps: device fp64 [ntaps], the filter h = firwin(2*half + 1, 1/M, window=("kaiser", 5.0)) * up with
 * M = max(up, down), half = 10*M (up-scaled, unpadded, ntaps odd, ntaps == 20*max(up,down)+1, or ntaps == 1 with
 * up == down == 1: decode and downmix only). With n_pre_pad = down - half % down and
 * n_pre_remove = (half + n_pre_pad) / down, output j of a row is
 *   y[j] = sum_i x[i] * h[c - i*up],  c = (j + n_pre_remove)*down - n_pre_pad,  0 <= i < n,  0 <= c - i*up < ntaps,
 * accumulated in fp64 fma in ascending i; a row's result does not depend on B or on the other rows.
 * d_y: fp64 [B][ldy], row b receives n_out[b] = ceil(n[b]*up/down) samples (host array out), the rest of the row is
 * zeroed so d_y is a valid input of rvcx_pipeline_batch_v. No model has to be loaded.
 * RVCX_E_INVALID: bad arguments (a null pointer, n[b] < 1 or > ldx, an unknown dtype, ntaps of another length).
 * RVCX_E_SHAPE: ldy below a row's n_out; up / down not positive and coprime; ceil(ntaps / up) above 8191 input
 * samples per output (a ratio whose filter does not fit the staged window, e.g. 1/410). */
int rvcx_resample_poly_v(rvcx_ctx* ctx, const void* d_x, int dtype, int channels, const int64_t* n, int64_t ldx, int B,
                         int up, int down, const double* d_taps, int64_t ntaps, double* d_y, int64_t ldy,
                         int64_t* n_out, void* stream);

/* Options of Pipeline.pipeline (rvc/infer/pipeline.py:390-408; rvc_mlx/infer/pipeline_mlx.py:263) that
 * reach the device path. Fill with rvcx_pipeline_default_opts, then override. Times are in samples. */
typedef struct {
  int sid;                          /* speaker id (emb_g row) */
  int version;                      /* 0 = from the synthesizer (768-d -> v2, 256-d -> v1), or 1 / 2 */
  double pitch;                     /* semitones, f0 *= 2^(pitch/12) (pipeline.py:278-279) */
  float protect;                    /* consonant protection, active when < 0.5 (pipeline.py:350-362) */
  float rmvpe_threshold;            /* decode threshold (0.03, pipeline.py:237) */
  int64_t t_pad, t_pad_tgt;         /* x_pad * 16000 and x_pad * tgt_sr (pipeline.py:176-177) */
  int64_t t_query, t_center, t_max; /* x_query/x_center/x_max * 16000: long-input split search (:440-452);
                                       t_max = 0 disables splitting */
  int f0_autotune;                  /* Autotune.autotune_f0 (pipeline.py:151-162, :248-249) */
  double f0_autotune_strength;
  int proposed_pitch;               /* key offset from the median f0 (pipeline.py:250-277) */
  double proposed_pitch_threshold;
  double volume_envelope;           /* AudioProcessor.change_rms rate; 1 = off (pipeline.py:545-549) */
  int mlx_semantics;                /* 1: f0 adjustments as rvc_mlx PipelineMLX.get_f0 (pipeline_mlx.py:135-164):
                                       autotune skips f0 <= 0 and the pitch shift is applied after it */
  double index_rate;                /* speaker-embedding retrieval blend (pipeline.py:338-342, :378-388); 0 = off;
                                       > 0 needs rvcx_index_load */
  int f0_method;                    /* 0 = RMVPE (default), 1 = CREPE with the loaded RVCX_MODEL_CREPE weights
                                       (PitchExtractor.extract, pitch_extractors.py:155-156; f0_min 50, f0_max
                                       1100, threshold 0.1), 2 = CREPE as rvc/ runs it (pipeline.py:223-234;
                                       rvcx_crepe_ex semantics 1, without the dither), 3 = FCPE with the loaded
                                       RVCX_MODEL_FCPE weights (rvc/lib/predictors/f0.py:77-87: the raw track,
                                       zeros where unvoiced; the model's hop must be 160 at 16 kHz), 4 = RMVPE with
                                       the rows of a batch in one ragged pass (rvcx_rmvpe_batch_v; in
                                       rvcx_pipeline_batch_v only: a row's f0 then equals method 0's up to summation
                                       order, not bit for bit. One utterance and equal lengths run as method 0),
                                       5 = FCPE with the rows of a batch in one ragged pass (rvcx_fcpe_batch_v; in
                                       rvcx_pipeline_batch_v only, method 3's requirements: a row's f0 then equals
                                       method 3's up to summation order. Equal lengths share rvcx_fcpe_b's batched
                                       pass; one utterance runs as method 3) */
  float fcpe_threshold;             /* FCPE's voicing threshold (FCPE.get_f0's filter_radius, f0.py:71); <= 0: 0.006 */
} rvcx_pipeline_opts;

/* Defaults of the rvc/ Config (x_pad 1, x_query 6, x_center 38, x_max 41; rvc/configs/config.py) at
 * 48 kHz, protect 0.33, volume_envelope 1. */
int rvcx_pipeline_default_opts(rvcx_pipeline_opts* opts);

/* Pipeline.pipeline, all on device (rvc/infer/pipeline.py:390-558 with pitch_guidance and
 * index_rate 0; rvc_mlx/infer/pipeline_mlx.py:263-373): filtfilt(audio) -> reflect pad t_pad -> RMVPE
 * -> get_f0 adjustments -> [split at the quietest points near every t_center when the input exceeds
 * t_max] -> voice_conversion per chunk -> trim t_pad_tgt per side -> concatenate -> change_rms ->
 * peak-normalise. d_audio [n] fp64 @16 kHz; out fp32 @tgt_sr, n_out samples (cap >=
 * ((n + 2 t_pad)/160 + n/t_center + 2) * upp is always enough). d_eps_z / d_eps_src (optional)
 * hold the injected noise of all chunks back to back ([192][T_i] then [T_i * upp] per chunk);
 * d_f0 (optional) receives the adjusted f0 [1 + (n + 2 t_pad)/160]. The host synchronises the
 * stream once to read the split points (long inputs only) and once for proposed_pitch.
 * The HiFi-GAN generator runs only over the frames whose samples the trim keeps, plus its receptive field: the
 * output is unchanged bit for bit from a full-length run (the trimmed samples were never returned). */
int rvcx_pipeline_ex(rvcx_ctx* ctx, const double* d_audio, int64_t n, const rvcx_pipeline_opts* opts,
                     const float* d_eps_z, const float* d_eps_src, uint64_t seed, float* d_out, int64_t cap,
                     int64_t* n_out, double* d_f0, void* stream);

/* Batched offline conversion (config C4): B equal-length utterances (each n + 160 <= t_max, i.e. one chunk),
 * d_audio row b at d_audio + b*lda (fp64 @16 kHz), sids host [B]. Every stage runs once for the whole batch
 * (batched RMVPE, HuBERT and Synthesizer.infer); row b of d_out (stride ldo) receives Pipeline.pipeline's
 * output for utterance b, n_out samples. Noise when injected: d_eps_z [B][inter][T], d_eps_src [B][T*upp].
 * Optional outputs: d_f0 [B][F] the adjusted f0 of each row (as rvcx_pipeline_ex's d_f0), d_hidden [B][F][360] the
 * RMVPE salience each row's f0 was decoded from (RMVPE f0 method only), F = 1 + (n + 2 t_pad)/160. CREPE and FCPE
 * (f0_method 1-3) run per row. As in rvcx_pipeline_ex the generator skips the frames the trim drops (one window for
 * all rows); outputs are unchanged bit for bit. */
int rvcx_pipeline_batch(rvcx_ctx* ctx, const double* d_audio, int64_t n, int64_t lda, int B,
                        const rvcx_pipeline_opts* opts, const int32_t* sids, const float* d_eps_z,
                        const float* d_eps_src, uint64_t seed, float* d_out, int64_t ldo, int64_t* n_out,
                        double* d_f0, float* d_hidden, void* stream);

/* rvcx_pipeline_batch for utterances of different lengths: row b has n[b] samples (host array; every n[b] + 160 <=
 * t_max, lda >= every n[b]); row b of d_out (stride ldo) receives Pipeline.pipeline's output for utterance b, n_out[b]
 * samples (host array; samples of a row past n_out[b], up to the longest row's count, may be overwritten). One ragged
 * HuBERT pass (rvcx_hubert_batch_v), one Synthesizer.infer with per-row lengths, and one launch set per stage for the
 * upsample + protect, the pitch packing, the trim, the volume envelope and the peak normalisation, whatever B is.
 * The pitch network runs per row under f0_method 0 (the default: a row's f0 is then rvcx_pipeline_ex's bit for bit),
 * rows of equal length inside the batch sharing one batched RMVPE pass; f0_method 4 runs all rows in one ragged RMVPE
 * pass (rvcx_rmvpe_batch_v: equal to the per-row pass up to summation order). FCPE likewise: per row under f0_method 3,
 * all rows in one ragged pass under f0_method 5 (rvcx_fcpe_batch_v).
 * Noise when injected uses rvcx_pipeline_batch's layouts with T the longest row's frame count T_max = max_b
 * min((n[b] + 2 t_pad) / 160, 2 L_b): d_eps_z [B][inter][T_max], d_eps_src [B][T_max*upp]; row b consumes
 * d_eps_z[b][:, :T_b] and the first T_b*upp source draws, the draws a B = 1 call on that row consumes.
 * d_f0 (optional): row b's adjusted f0, 1 + (n[b] + 2 t_pad)/160 values at d_f0 + b*ldf.
 * The generator runs over the window common to all rows on z * mask, as the reference's batched Synthesizer.infer
 * does, so the last frames of a shorter row within the generator's receptive field (10 frames for the 48 kHz v2
 * model) differ from a run of that row alone; the trim removes them when t_pad_tgt covers that field. Rows of
 * different lengths with a smaller t_pad_tgt fail with RVCX_E_INVALID. Equal lengths take rvcx_pipeline_batch's
 * stages. rvcx_workspace_bytes(B, n_max, opts) sizes an arena for a ragged batch of B rows with every n[b] <= n_max:
 * it also runs this call on B rows of n_max as a ragged batch, and adds room for the shared split-K slab to be regrown
 * once per row. */
int rvcx_pipeline_batch_v(rvcx_ctx* ctx, const double* d_audio, const int64_t* n, int64_t lda, int B,
                          const rvcx_pipeline_opts* opts, const int32_t* sids, const float* d_eps_z,
                          const float* d_eps_src, uint64_t seed, float* d_out, int64_t ldo, int64_t* n_out,
                          double* d_f0, int64_t ldf, void* stream);

/* rvcx_pipeline_batch_v with a voice per row (the voice bank below): voices host [B], NULL = every row on the current
 * voice, which is rvcx_pipeline_batch_v itself, bit for bit (rvcx_pipeline_batch_v and rvcx_pipeline_batch are this
 * call with voices = NULL). The rows of one voice must be contiguous (RVCX_E_INVALID; the host sorts), every voice must
 * exist (RVCX_E_INVALID) and be finalized (RVCX_E_STATE), and the voices must agree on sr, the product of the upsample
 * rates, text_enc_hidden_dim, inter_channels, no_f0 and vocoder (RVCX_E_SHAPE). sids[b] is checked against row b's
 * voice; index_rate > 0 needs an index on every voice in the batch (RVCX_E_STATE). The high-pass, the ragged HuBERT, the
 * pitch network (any f0_method) and the f0 adjustments run once over all rows -- they do not depend on the voice, so
 * under f0_method 0 a row's f0 is still the single run's bit for bit; retrieval (against each voice's own index) and
 * Synthesizer.infer with per-row lengths and the common output window run once per voice on its row range at the
 * batch's strides; the trim, the volume envelope and the peak normalisation once. Rows of different lengths need
 * t_pad_tgt to cover the widest receptive field among the voices' generators. With several voices, injected source
 * noise needs the HiFi-GAN-NSF layout (one row per batch row), and drawn noise (no d_eps_*) is keyed by the row within
 * its voice's range under a seed derived from `seed` and the range's first row. The context's current voice is the
 * same after the call as before, on an error too. */
int rvcx_pipeline_batch_voices(rvcx_ctx* ctx, const double* d_audio, const int64_t* n, int64_t lda, int B,
                               const rvcx_pipeline_opts* opts, const int32_t* sids, const int32_t* voices,
                               const float* d_eps_z, const float* d_eps_src, uint64_t seed, float* d_out, int64_t ldo,
                               int64_t* n_out, double* d_f0, int64_t ldf, void* stream);

/* Single-chunk shorthand of rvcx_pipeline_ex (t_max = 0, defaults otherwise). */
int rvcx_pipeline(rvcx_ctx* ctx, const double* d_audio, int64_t n, int sid, double semitones, float protect,
                  int64_t t_pad, int64_t t_pad_tgt, const float* d_eps_z, const float* d_eps_src, uint64_t seed,
                  float* d_out, int64_t cap, int64_t* n_out, double* d_f0, void* stream);

/* Device workspace (SURVEY.md 8(b) "Ownership"; replaces nothing in the reference, whose MLX / torch allocators own
 * all scratch). Every intermediate of a call (activations, split-K slabs, filter state, attention partials ...) lives
 * in the context's named pool, allocated on first use and kept across calls; the weights and their pre-split images
 * are not part of it.
 * rvcx_workspace_bytes: the pool a pipeline call of B utterances of n samples under opts takes (B = 1 as
 *   rvcx_pipeline_ex, B > 1 as rvcx_pipeline_batch). It runs that call once on zero audio on `stream` from an empty
 *   pool (loaded models required; outputs discarded) and reports every region the pool took, regrown ones included,
 *   so an arena of that size holds the call; the pool is released again before it returns. Inputs above t_max are
 *   sized on the worst-case split plan (the longest chunk any audio can give: the pipeline processes its chunks
 *   longest first, so the work buffers grow only inside the first chunk), so the size holds for any audio of n samples.
 *   With f0_method 3 the FCPE network's scratch (mel, activations, the attention's ctx / ksum slab images) is carved
 *   in place of RMVPE's; the call is then sized under f0_method 0 as well and the larger size is reported.
 *   With f0_method 4 and B > 1 the ragged RMVPE pass is sized on B rows of n samples; with f0_method 5 the ragged
 *   FCPE pass, and as under f0_method 3 the size also covers the same call under f0_method 0.
 *   The query is made for the current voice. A call with a voice per row (rvcx_pipeline_batch_voices) is held by an
 *   arena of the maximum of rvcx_workspace_bytes(B, n_max, opts) over the voices in use (select each, ask, take the
 *   largest): the per-voice stages run on row ranges of at most B rows, the largest range first, in the buffers the
 *   whole batch would take.
 * rvcx_set_workspace: hand the context a caller-owned device arena (e.g. a torch uint8 tensor's data_ptr(), 256-B
 *   aligned), valid until replaced or the context is destroyed: the pool is then carved from it and never allocated,
 *   and a call that would need more fails with RVCX_E_OOM. NULL, 0 returns to internal allocation. The current pool
 *   is released first (the device is synchronised). While attached the arena belongs to the library: every compute
 *   call carves its regions from offset 0 again (a sized arena then holds any sequence of calls each of which it
 *   holds alone), and nothing is assumed to survive between calls, so a caller's writes into the arena between calls
 *   cannot change results -- but they must be stream-ordered after the previous call's work.
 * rvcx_workspace_info: bytes the pool holds now, the arena size and the arena bytes carved so far (any may be NULL). */
int rvcx_workspace_bytes(rvcx_ctx* ctx, int B, int64_t n, const rvcx_pipeline_opts* opts, int64_t* bytes,
                         void* stream);
int rvcx_set_workspace(rvcx_ctx* ctx, void* d_base, int64_t bytes);
int rvcx_workspace_info(const rvcx_ctx* ctx, int64_t* held, int64_t* arena_bytes, int64_t* arena_used);

/* Kernel timing for roofline reporting: when enabled, every implicit-GEMM conv launch (the MFMA
 * kernel family that carries ~all FLOPs) is bracketed by hipEvents recorded on its own stream.
 * rvcx_profile_read synchronises those events and returns the summed kernel time (ms), the
 * summed ALGORITHMIC FLOPs of those launches and the launch count, then clears the record. */
int rvcx_profile(rvcx_ctx* ctx, int enable);

/* Synchronise `stream` (and the context's internal side stream) and report device-side faults raised by
 * kernels of earlier calls: RVCX_E_HIP when, e.g., the RMVPE BiGRU's cross-workgroup hand-off timed out (its
 * outputs are then invalid). The flags are cleared once reported. Every compute entry point also reports
 * flags of already-completed calls on entry, and the pipeline checks them at its own synchronisation points.
 * (Replaces nothing in the reference, whose computations cannot fail this way; it never prints and continues.) */
int rvcx_device_status(rvcx_ctx* ctx, void* stream);
int rvcx_profile_read(rvcx_ctx* ctx, double* total_ms, double* total_flops, int64_t* launches);
/* As rvcx_profile_read, plus the launches' time at their arithmetic's MFMA ceiling (ms): sum of flops / ceiling,
 * with the ceiling 2500 / 6 TF for the exact bf16 split, 2500 / 3 for the two-plane fp16 split and 2500 for the fp16
 * reduced-precision mode (the dense bf16 / fp16 MFMA peak over the MFMA products per fp32 product). */
int rvcx_profile_read_ex(rvcx_ctx* ctx, double* total_ms, double* total_flops, int64_t* launches, double* ceiling_ms);
/* As rvcx_profile_read_ex, plus the same sums per kernel family (the kernel each launch actually ran, after routing):
 * arrays of nk entries indexed by family id (0 .. RVCX_PROF_KINDS - 1; names from rvcx_profile_kind_name), each
 * with the summed event time (ms), algorithmic FLOPs, time at the arithmetic's ceiling (ms), algorithmic HBM bytes
 * (operands read once, result written once) and launch count. A family's time includes its split-K combine. */
#define RVCX_PROF_KINDS 10
int rvcx_profile_read_kinds(rvcx_ctx* ctx, double* total_ms, double* total_flops, int64_t* launches, double* ceiling_ms,
                            int nk, double* k_ms, double* k_flops, double* k_ceiling_ms, double* k_bytes,
                            int64_t* k_launches);
const char* rvcx_profile_kind_name(int kind);

/* ---------------------------------------------------------------- feature index (FAISS IndexIVFFlat)
 * The bytes of a faiss .index file (IndexIVFFlat over IndexFlatL2, METRIC_L2, ArrayInvertedLists;
 * faiss 1.7.4 write_index layout). Replaces faiss.read_index + index.reconstruct_n(0, ntotal) at
 * rvc/infer/pipeline.py:430-434 (rvc_mlx/infer/pipeline_mlx.py:267-278). The lists, centroids and ids
 * are kept in HBM; nprobe comes from the file. ids must be a permutation of 0..ntotal-1 (RVC indexes). */
int rvcx_index_load(rvcx_ctx* ctx, const void* bytes, int64_t nbytes);
int rvcx_index_unload(rvcx_ctx* ctx);
/* Validate a faiss .index image on the host only (no context, no device): the same parser rvcx_index_load runs.
 * Fills d/ntotal/nlist/nprobe (each optional); on failure writes the message to err (err_cap bytes). Every size
 * in the file is untrusted: counts are checked against the bytes left and list sizes against ntotal. */
int rvcx_index_parse(const void* bytes, int64_t nbytes, int64_t* d, int64_t* ntotal, int64_t* nlist, int64_t* nprobe,
                     char* err, int64_t err_cap);
/* RVCX_E_STATE when no index is loaded. */
int rvcx_index_info(const rvcx_ctx* ctx, int64_t* d, int64_t* ntotal, int64_t* nlist, int64_t* nprobe);
/* faiss.extract_index_ivf(index).nprobe = nprobe (clamped to nlist). */
int rvcx_index_set_nprobe(rvcx_ctx* ctx, int64_t nprobe);
/* index.search(x, k) (IndexIVF::search, L2; used at pipeline.py:380 with k = 8): d_x [n][d] fp32 ->
 * d_dist [n][k] fp32 squared L2, d_ids [n][k] int64, ordered by (distance, id), (+inf, -1) padding. k <= 16. */
int rvcx_index_search(rvcx_ctx* ctx, const float* d_x, int64_t n, int k, float* d_dist, int64_t* d_ids,
                      void* stream);
/* index.reconstruct_n(i0, ni) -> d_out [ni][d] (big_npy rows, pipeline.py:434). */
int rvcx_index_reconstruct_n(rvcx_ctx* ctx, int64_t i0, int64_t ni, float* d_out, void* stream);
/* Pipeline._retrieve_speaker_embeddings (pipeline.py:378-388): d_feats [L][d] -> d_out [L][d] =
 * index_rate * sum_j w_j big_npy[ix_j] + (1 - index_rate) * feats, w = (1/dist)^2 normalised, k = 8,
 * with numpy/torch float32 rounding. */
int rvcx_index_retrieve(rvcx_ctx* ctx, const float* d_feats, int64_t L, int d, double index_rate, float* d_out,
                        void* stream);

/* ---------------------------------------------------------------- feature index: build and write
 * Replaces faiss.index_factory(768, f"IVF{n_ivf},Flat") + train + add + faiss.write_index of
 * rvc/train/process/extract_index.py:58-70 (faiss-cpu k-means + IndexIVF::add) on device. Unpinned against faiss
 * itself (its random choices cannot be reproduced); the deviations are listed in csrc/index_build.cpp. */
typedef struct {
  int niter;                /* Lloyd iterations; 10 = faiss's cp.niter for the IVF coarse quantizer (train, :64) */
  int64_t nprobe;           /* nprobe of the built index; 1 as extract_index.py:63 */
  uint64_t seed;            /* seeds the choice of the initial centroids when init_rows is NULL */
  const int64_t* init_rows; /* host, nlist distinct rows of d_x: the initial centroids; NULL = drawn from seed */
} rvcx_index_build_opts;
/* niter 10, nprobe 1, seed 0, init_rows NULL. Returns rvcx_status like every entry here (RVCX_E_INVALID for NULL). */
int rvcx_index_default_build_opts(rvcx_index_build_opts* o);
/* index.train(big_npy) + index.add(big_npy) (extract_index.py:64-68): k-means over d_x [n][d] fp32 (device, 16-byte
 * aligned; d a multiple of 64 up to 1024, else RVCX_E_SHAPE) into nlist centroids, then every row, id = its row
 * number, into the list of its nearest centroid. The result becomes the context's loaded index exactly as
 * rvcx_index_load leaves it (a previously loaded index is replaced only when the build succeeds). Synchronises
 * `stream` once per iteration. opts NULL = the defaults. RVCX_E_INVALID for nlist < 1, nlist > n, niter < 0,
 * nprobe < 1 or duplicate / out-of-range init_rows. */
int rvcx_index_build(rvcx_ctx* ctx, const float* d_x, int64_t n, int d, int64_t nlist,
                     const rvcx_index_build_opts* opts, void* stream);
/* The loaded index's coarse centroids -> d_out [nlist][d] (faiss: index.quantizer.reconstruct_n(0, nlist)); the
 * k-means reduction of extract_index.py:46-56 reads them back. RVCX_E_STATE when no index is loaded. */
int rvcx_index_centroids(rvcx_ctx* ctx, float* d_out, void* stream);
/* faiss.write_index(index, path) (extract_index.py:70) into host memory: the loaded index, built here or loaded
 * from a file, as faiss 1.7.4 IndexIVFFlat bytes (direct map type 0; "full" list sizes when more than nlist / 2
 * lists are non-empty, else "sprs"; an index loaded from a file keeps that file's choice of the two, so it saves
 * back byte for byte). *nbytes = the size; bytes NULL reports only the size. RVCX_E_CAPACITY when cap is too
 * small, RVCX_E_STATE when no index is loaded. Synchronises the device. */
int rvcx_index_save(rvcx_ctx* ctx, void* bytes, int64_t cap, int64_t* nbytes);

/* ---------------------------------------------------------------- streaming (config C5)
 * A group of n_streams concurrent realtime streams of one buffer geometry, converted together per hop.
 * Replaces VoiceChanger / Realtime / Realtime_Pipeline of rvc/realtime/core.py:329-484 and
 * rvc/realtime/pipeline.py:99-334 (the MLX port of this path, rvc_mlx/realtime, is not functional).
 * Geometry follows VoiceChanger.__init__ + Realtime.realloc (core.py:165-216, :351-374): block =
 * read_chunk_size * 128 samples @48 kHz; convert buffer = block + sola (10 ms) + extra + crossfade
 * @16 kHz rounded up to 10 ms; skip_head = extra / 10 ms; return_length = frames - skip_head. */
typedef struct rvcx_rt rvcx_rt;

typedef struct {
  int n_streams;                  /* B streams per hop batch */
  int read_chunk_size;            /* block = read_chunk_size * 128 samples @48 kHz (callbacks.py default 192) */
  double cross_fade_overlap_size; /* seconds (default 0.1) */
  double extra_convert_size;      /* seconds (default 0.5) */
  double silent_threshold;        /* dB; hops with RMS below 10^(dB/20) output silence (core.py:58-59, :268-289) */
  int f0_method;                  /* VoiceChanger's f0_method (pipeline.py:140-155): 0 "rmvpe" (a zero-initialised desc),
                                   * 1 "fcpe": one batched FCPE forward per hop, the raw local_argmax track */
  float fcpe_threshold;           /* f0_method 1: FCPE's voicing threshold; <= 0: 0.006 (pipeline.py:155) */
} rvcx_rt_desc;

typedef struct {                  /* per-hop options of VoiceChanger.on_request (core.py:453-484); one for the group
                                   * (rvcx_rt_process) or one per stream (rvcx_rt_process_v) */
  double f0_up_key;
  double index_rate;              /* > 0 needs rvcx_index_load; retrieval from skip_head // 2 */
  float protect;                  /* active when < 0.5 */
  double volume_envelope;         /* 1 = off */
  int f0_autotune;
  double f0_autotune_strength;
  int proposed_pitch;             /* one host sync per hop */
  double proposed_pitch_threshold;
  int gen_precision;              /* 0 (default) fp32-accurate everywhere; 1 = this hop's GENERATOR (HiFi-GAN-NSF
                                   * decoder: its weight-streamed convs and 32-channel fused ResBlock pairs) on fp16
                                   * operands with fp32 accumulation, one MFMA product per step: BASELINE C5's fp16
                                   * streaming. RMVPE, HuBERT, the TextEncoder and the flow stay fp32-accurate, and no
                                   * other entry point is affected (the setting travels with the hop, not the ctx). */
} rvcx_rt_opts;

int rvcx_rt_default_desc(rvcx_rt_desc* desc);
int rvcx_rt_default_opts(rvcx_rt_opts* opts);
/* Needs the synthesizer and HuBERT finalized and, for a pitch-guided synthesizer, the f0 method's model: RMVPE
 * (f0_method 0) or RVCX_MODEL_FCPE at 16 kHz / hop_size 160 (f0_method 1; RVCX_E_STATE / RVCX_E_SHAPE otherwise). Any
 * other f0_method: RVCX_E_INVALID. State lives in HBM, zero-initialised. */
int rvcx_rt_create(rvcx_ctx* ctx, const rvcx_rt_desc* desc, rvcx_rt** out);
int rvcx_rt_destroy(rvcx_ctx* ctx, rvcx_rt* rt);
/* geometry[12] = {n_streams, block48, block16, convert16, frames (p_len), skip_head, return_length,
 *                 crossfade48, sola_search48, extra48, resampled_block16, silence_front} */
int rvcx_rt_geometry(const rvcx_rt* rt, int64_t* geometry);
int rvcx_rt_reset(rvcx_ctx* ctx, rvcx_rt* rt, void* stream);
/* One hop for every stream: d_in [B][block48] fp32 @48 kHz -> d_out [B][block48] fp32 @48 kHz
 * (VoiceChanger.process_audio). sids: host [B]. d_vol (optional, device [B]) receives each stream's
 * input RMS (the `vol` of on_request); d_offs (optional, device int [B]) the SOLA offsets. Noise: d_eps_z
 * [B][inter][frames] and d_eps_src [B][frames * upp] when injected, else Philox(seed). */
int rvcx_rt_process(rvcx_ctx* ctx, rvcx_rt* rt, const float* d_in, const int32_t* sids, const rvcx_rt_opts* opts,
                    const float* d_eps_z, const float* d_eps_src, uint64_t seed, float* d_out, float* d_vol,
                    int32_t* d_offs, void* stream);
/* rvcx_rt_process with one rvcx_rt_opts per stream and an optional set of idle slots.
 * opts: host [B]. active: host [B] (0 = idle this hop), NULL = all active. rvcx_rt_process(o) is this call with B
 * copies of o and active = NULL.
 * Per-stream options: each stream gets its own on_request arguments -- its own pitch factor (f0_up_key, and the
 * proposed key when proposed_pitch is set and autotune is not; the host syncs once, and only on hops where an active
 * stream asks), autotune on its own f0 row only (factor 1 there, the other rows' f0 bits untouched), protect, index_rate
 * (one batched search over every stream that retrieves, each blended at its own (float)r / (float)(1 - r); streams at
 * rate 0 are copied through) and volume_envelope (one batched change_rms; streams at exactly 1 untouched).
 * gen_precision belongs to the hop: the active streams must agree (RVCX_E_INVALID). RVCX_E_STATE when an active
 * stream has index_rate > 0 and no index is loaded. Nothing is launched and no state changes when the call fails so.
 * Idle slots: for a slot with active[b] == 0 the hop did not happen -- its row of d_in is not read, none of its state
 * changes, its d_out row is zeros, its d_vol 0 and its d_offs 0; its opts and sid are ignored. The networks run on the
 * active streams only, compacted in slot order; with no active stream the call only writes the zero outputs.
 * Noise: injected d_eps_z / d_eps_src are indexed by SLOT (row b belongs to slot b, idle rows are not read; with idle
 * slots the injected source noise needs the HiFi-GAN-NSF layout, one [frames * upp] row per slot, else
 * RVCX_E_INVALID). Drawn noise (Philox(seed)) is keyed by COMPACT ROW, the stream's position among the active ones:
 * the draws of a hop are distinct across its active streams, and a stream's draws for one seed move when a
 * lower-numbered slot goes idle -- vary the seed per hop, as VoiceChanger does. */
int rvcx_rt_process_v(rvcx_ctx* ctx, rvcx_rt* rt, const float* d_in, const int32_t* sids, const rvcx_rt_opts* opts,
                      const uint8_t* active, const float* d_eps_z, const float* d_eps_src, uint64_t seed,
                      float* d_out, float* d_vol, int32_t* d_offs, void* stream);
/* Realtime(..., clean_audio, clean_strength) (rvc/realtime/core.py:86-94: arguments of the constructor, not of
 * on_request) for one stream of the group, or for all of them with stream_index = -1: clean_audio != 0 sends that
 * stream's model output through the noise gate (rvcx_spectral_gate at the model's sampling rate, prop_decrease =
 * clean_strength) on every hop from now on, 0 (the state a group is created in) turns it off. A setting of the slot,
 * like its sid: rvcx_rt_reset and rvcx_rt_reset_stream leave it, and rvcx_rt_opts keeps its layout.
 * The rows that clean are gated after the clip and the volume envelope and before the sqrt(vol) scale, the output
 * resample and SOLA, as pipeline.py:326-327 does; the other rows and idle slots are untouched. The gate's statistics
 * run over the whole model row, so on a hop where an active stream cleans the generator runs full-length (no output
 * window). gen_precision is independent of it.
 * RVCX_E_INVALID, with no stream's setting changed and nothing launched, for a stream_index outside [-1, n_streams),
 * a clean_strength outside [0, 1], a model row (frames * upp) shorter than 2048 samples, or a geometry in which a
 * sample SOLA reads (through the output resampler's kernel when the model does not run at 48 kHz) would come from the
 * gate's zeroed tail [256 * (n_model / 256), n_model): a hop therefore never meets a setting it has to refuse. */
int rvcx_rt_set_clean(rvcx_ctx* ctx, rvcx_rt* rt, int stream_index, int clean_audio, double clean_strength);

/* The noise gate on its own: noisereduce.torchgate.TorchGate(sr, nonstationary=False, prop_decrease=strength) as
 * rvc/realtime/core.py:86-94 builds it and rvc/realtime/pipeline.py:326-327 calls it (no separate noise clip):
 * STFT (n_fft = win = 1024, hop 256, periodic Hann, centred with zero padding), per (row, bin) a threshold of
 * mean + 1.5 std (unbiased) over the frames of 20 log10(|X| + eps) clamped to its maximum - 40 dB, the mask
 * smoothed by the 500 Hz x 50 ms triangle filter, inverse STFT.
 * d_x [B][n] (rows ldx apart) -> d_y [B][n] (rows ldy apart): samples [0, n_out), n_out = 256 * (n / 256), are the
 * gate's output (torch.istft's length) and samples [n_out, n) are written as zeros. strength: host [B], each row's
 * prop_decrease in [0, 1]; a negative entry copies that row through unchanged (all n samples). d_mask (optional):
 * [B][513][1 + n / 256] bytes, 1 where a bin is above its threshold (rows copied through are not written).
 * All rows share each launch (four launches whatever B is); the overlap-add is a fixed-order gather, so a call gives
 * the same bits every time. RVCX_E_SHAPE for n < 2048 or an sr whose smoothing filter is empty (int(500 / (sr / 512))
 * < 1 or int(50 / (256 / sr * 1000)) < 1), RVCX_E_INVALID for a strength above 1; nothing is launched then. */
int rvcx_spectral_gate(rvcx_ctx* ctx, const float* d_x, int B, int64_t n, int64_t ldx, int sr, const float* strength,
                       float* d_y, int64_t ldy, uint8_t* d_mask, void* stream);

/* rvcx_rt_reset for one slot: its audio / convert / pitch / pitchf buffers and SOLA tail zeroed, asynchronous on
 * `stream`, the other slots untouched. RVCX_E_INVALID when stream_index is not in [0, n_streams). */
int rvcx_rt_reset_stream(rvcx_ctx* ctx, rvcx_rt* rt, int stream_index, void* stream);

/* The effective configuration as a NUL-terminated JSON object (cap bytes; *len, optional, gets its length): the
 * context's contraction arithmetic, whether developer knobs are enabled, and every RVCX_* environment variable of the
 * process with whether it is honoured. The RVCX_* tuning / A-B switches (tile and split-K policy, kernel-path and
 * arithmetic overrides such as RVCX_CONV_MATH) are read only when RVCX_EXPERIMENTAL=1: without it they are ignored and
 * listed here as not honoured. RVCX_E_CAPACITY when cap is too small (the string is truncated). ctx may be NULL (the
 * process-wide fields only; no device is touched). */
int rvcx_config_info(const rvcx_ctx* ctx, char* buf, int64_t cap, int64_t* len);

/* Upsampling factor of the loaded synthesizer (prod(upsample_rates); net_g.dec.upp). */
int rvcx_synth_upp(const rvcx_ctx* ctx);

/* Voice bank: several voice models resident in one context.
 * A voice is everything that differs between two RVC checkpoints: the synthesizer configuration, the uploaded and
 * packed RVCX_MODEL_SYNTH tensors with the pre-split weight images derived from them, and the feature index with its
 * nprobe. HuBERT, RMVPE, CREPE, FCPE, the high-pass, the workspace and the profile belong to the context and are shared.
 * The context has a CURRENT voice. Voice 0 exists from rvcx_create and is current; every entry point that reads or
 * writes "the" synthesizer or "the" index (rvcx_set_synth_config, rvcx_upload / rvcx_finalize of RVCX_MODEL_SYNTH,
 * rvcx_synth_*, rvcx_dec_only, rvcx_voice_conversion, rvcx_pipeline*, rvcx_index_*, rvcx_workspace_bytes,
 * rvcx_rt_create) acts on the current voice.
 * rvcx_voice_new: adds an empty voice and returns its id; the current voice stays. Ids are never reused within a
 *   context, so a stale id is detected.
 * rvcx_voice_select: host only -- no device call, no synchronisation, no copy of weight data. RVCX_E_INVALID for an
 *   unknown or freed id. Like every other call on a context it must not run concurrently with another call on it.
 * rvcx_voice_info: any live voice, current or not.
 * rvcx_voice_free: synchronises the device, then releases the voice's tensors, the split images built from them and its
 *   index. RVCX_E_STATE for voice 0 and for the current voice, RVCX_E_INVALID for an unknown or freed id. */
typedef struct {
  rvcx_synth_desc synth; /* as set; zeros before rvcx_set_synth_config */
  int config_set;        /* rvcx_set_synth_config was called for this voice */
  int ready;             /* RVCX_MODEL_SYNTH finalized */
  int64_t index_d, index_ntotal, index_nlist, index_nprobe; /* zeros without an index */
  int64_t weight_bytes;  /* the packed tensors in HBM */
  int64_t split_bytes;   /* the pre-split weight images built from them so far (they are built on first use) */
} rvcx_voice_desc;
int rvcx_voice_new(rvcx_ctx* ctx, int* voice);
int rvcx_voice_select(rvcx_ctx* ctx, int voice);
int rvcx_voice_current(const rvcx_ctx* ctx, int* voice);
int rvcx_voice_info(rvcx_ctx* ctx, int voice, rvcx_voice_desc* desc);
int rvcx_voice_free(rvcx_ctx* ctx, int voice);

/* A voice per stream slot. rvcx_rt_create takes its geometry from the current voice and starts every slot on it; a
 * slot's voice then stays with the slot whatever rvcx_voice_select does later, and a hop leaves the context's current
 * voice as it found it, on an error too.
 * rvcx_rt_set_voice (stream_index -1 = every slot): the voice must agree with the group's geometry voice on sr, the
 *   product of the upsample rates, text_enc_hidden_dim, inter_channels, no_f0 and vocoder (what fixes the buffer
 *   geometry, the HuBERT version and the layout of injected noise), else RVCX_E_SHAPE; RVCX_E_INVALID for an unknown or
 *   freed id or a stream_index outside [-1, n_streams), RVCX_E_STATE for a voice that is not finalized. A refused call
 *   changes no slot. The slot's state is not cleared: a newcomer calls rvcx_rt_reset_stream, a user who switches voice
 *   keeps the SOLA crossfade.
 * rvcx_rt_get_voices: out [n_streams].
 * The hop (rvcx_rt_process*) runs its front end (ingest, the pitch network, the f0 adjustments, HuBERT) once over all
 * active rows. The compact rows are ordered by voice: groups by their lowest active slot, rows within a group by slot
 * (one voice in use: slot order, as before). Retrieval (against that voice's index), upsample + protect and one
 * Synthesizer.infer then run per voice on its contiguous row range, and the hop's tail (volume envelope, gate,
 * resample, SOLA) once. sids[b] is checked against the slot's voice; index_rate > 0 on a slot whose voice has no index
 * and a freed voice in an active slot give RVCX_E_STATE (the group is usable again after rvcx_rt_set_voice). Drawn
 * noise is keyed by the row within its voice's range, under a seed derived from `seed` and the range's first row (one
 * voice in use: by compact row under `seed`, as before). With more than one voice in a hop, injected source noise
 * needs the HiFi-GAN-NSF layout (as with idle slots). */
int rvcx_rt_set_voice(rvcx_ctx* ctx, rvcx_rt* rt, int stream_index, int voice);
int rvcx_rt_get_voices(const rvcx_rt* rt, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* RVCX_H_ */
