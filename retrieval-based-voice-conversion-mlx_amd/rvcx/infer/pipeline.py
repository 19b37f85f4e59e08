"""PipelineMLX-compatible conversion pipeline on MI355X.

Mirrors the plugin surface of rvc_mlx/infer/pipeline_mlx.py (PipelineMLX, :84-373) and the
semantics of its PyTorch oracle rvc/infer/pipeline.py (Pipeline, :165-558): same constructor,
same ``pipeline`` / ``get_f0`` / ``voice_conversion`` signatures, numpy in and out. The work
runs in librvcx.so on the GPU (see include/rvcx.h); this module only converts arguments.

Semantics: ``semantics="rvc"`` (default) follows rvc/infer/pipeline.py -- t_pad = x_pad * 16000,
autotune replaces the pitch shift, long inputs are split at quiet points (x_query/x_center/x_max).
``semantics="mlx"`` applies the two documented deltas of the MLX port that are pure pipeline
policy: t_pad forced to 1600 samples (pipeline_mlx.py:318) and the MLX get_f0 order (autotune
skips f0 <= 0, then the shift is applied; pipeline_mlx.py:142-147). Differences the reference
marks as port bugs (zeroed flow noise, no opt_ts split) are not reproduced.

Errors raise (the reference prints and continues, pipeline_mlx.py:280-281).
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

from .models import CREPE, FCPE, HubertModel, RMVPE0Predictor, Synthesizer, _np


class Config:
    """rvc_mlx/configs/config.py:7-20 (x_pad, x_query, x_center, x_max in seconds)."""

    def __init__(self, x_pad=1, x_query=6, x_center=38, x_max=41):
        self.device = "rocm"
        self.gpu_name = "AMD Instinct MI355X"
        self.x_pad, self.x_query, self.x_center, self.x_max = x_pad, x_query, x_center, x_max
        self.is_half = False

    def device_config(self):
        return self.x_pad, self.x_query, self.x_center, self.x_max


class VoiceRef:
    """One resident voice as pipeline_many takes it per utterance: the engine's voice id (Engine.add_voice) and what the
    reference reads from the checkpoint for a call -- tgt_sr, pitch_guidance (cpt["f0"]), version -- plus the voice's
    own .index file (None: none)."""

    def __init__(self, id: int, tgt_sr: int, pitch_guidance: bool = True, version: str = "v2", file_index=None):
        self.id, self.tgt_sr, self.pitch_guidance = int(id), int(tgt_sr), bool(pitch_guidance)
        self.version, self.file_index = version, file_index


def voice_key(cfg, retrieves: bool):
    """What the voices of one batched pass must share (rvcx_pipeline_batch_voices): the sampling rate, the upsample
    product, the embedding width, inter_channels, pitch guidance and the vocoder of the synthesizer -- and, since a
    batch has one index_rate, whether the voice retrieves at all. cfg: a SynthConfig."""
    return (int(cfg.sr), int(np.prod(cfg.upsample_rates)), int(cfg.text_enc_hidden_dim), int(cfg.inter_channels),
            bool(cfg.use_f0), str(cfg.vocoder), bool(retrieves))


# pipeline_many's defaults: the best setting measured on a 64-utterance job of 2-30 s clips
# (profiles/ragged_batch_times.txt: 829.5 ms against 850.1 ms, 848.0 .. 850.8, for the per-utterance loop)
DEFAULT_BATCH = 8
DEFAULT_MAX_PAD = 0.125


class PipelineRVCX:
    # pipeline_mlx.py:82 / pitch_extractors.py:44 minus the pyworld CPU methods (dio, pm, harvest). "crepe" and
    # "crepe-tiny" run CREPE as each side defines it: semantics="mlx" as rvc_mlx/lib/mlx/crepe.py (reflect padding,
    # biased std, weighted-argmax decode), semantics="rvc" as rvc/lib/predictors/f0.py:31-55 (torchcrepe.predict:
    # zero padding, unbiased std, viterbi decode; its triangular dither of the decoded cents only with
    # crepe_dither=True in get_f0, as it is random; pipeline() decodes without it). "fcpe": with semantics="rvc" the FCPE
    # network of rvc/lib/predictors/FCPE.py on device, from the checkpoint passed as fcpe_weights (rvc/'s FCPE.get_f0,
    # rvc/lib/predictors/f0.py:59-89: the raw local_argmax track at fcpe_threshold, zeros where unvoiced; without
    # fcpe_weights it raises: torchfcpe's bundled model is not readable here); with semantics="mlx" the MLX stub's RMVPE
    # at threshold 0.006 x 5 (rvc_mlx/lib/mlx/fcpe.py:129-132), whatever weights are given.
    SUPPORTED_F0_METHODS = ("rmvpe", "crepe", "crepe-tiny", "fcpe")

    def __init__(self, tgt_sr, config, hubert_model: Optional[HubertModel] = None,
                 rmvpe_model: Optional[RMVPE0Predictor] = None, f0_method: str = "rmvpe", semantics: str = "rvc",
                 crepe_weights=None, crepe_dither: bool = False, fcpe_weights=None, fcpe_threshold: float = 0.006):
        if semantics not in ("rvc", "mlx"):
            raise ValueError("semantics must be 'rvc' or 'mlx'")
        self.x_pad, self.x_query, self.x_center, self.x_max = config.x_pad, config.x_query, config.x_center, \
            config.x_max
        self.sample_rate = 16000
        self.tgt_sr = int(tgt_sr)
        self.window = 160
        self.t_pad = int(self.sample_rate * self.x_pad)
        self.t_pad_tgt = int(self.tgt_sr * self.x_pad)
        self.t_pad2 = self.t_pad * 2
        self.t_query = int(self.sample_rate * self.x_query)
        self.t_center = int(self.sample_rate * self.x_center)
        self.t_max = int(self.sample_rate * self.x_max)
        self.time_step = self.window / self.sample_rate * 1000
        self.f0_min, self.f0_max = 50, 1100
        self.f0_mel_min = 1127 * np.log(1 + self.f0_min / 700)
        self.f0_mel_max = 1127 * np.log(1 + self.f0_max / 700)
        self.hubert_model = hubert_model
        self.rmvpe_model = rmvpe_model
        self.semantics = semantics
        self.crepe_dither = bool(crepe_dither)
        # {"full": path-or-state, "tiny": ...} (or one path for "full"); None = $RVCX_CREPE_DIR/crepe_{model}.npz
        self.crepe_weights = crepe_weights if isinstance(crepe_weights, dict) or crepe_weights is None \
            else {"full": crepe_weights}
        # a checkpoint path of rvc/lib/predictors/FCPE.py's format, or its (state, config) pair; None = no FCPE network
        self.fcpe_weights = fcpe_weights
        self.fcpe_threshold = float(fcpe_threshold)
        self._check_method(f0_method)
        self._f0_method = f0_method
        self.engine = (hubert_model or rmvpe_model).engine if (hubert_model or rmvpe_model) else None
        self.last_f0 = None

    # ------------------------------------------------------------------ helpers
    def _check_method(self, m):
        if m not in self.SUPPORTED_F0_METHODS:
            raise ValueError(f"f0_method {m!r} is not supported on this path (supported: {self.SUPPORTED_F0_METHODS})")
        if m == "fcpe" and self.semantics != "mlx" and self.fcpe_weights is None:
            raise ValueError("f0_method 'fcpe' on the rvc/ path (rvc/lib/predictors/f0.py:59-89) runs the FCPE network: "
                             "pass fcpe_weights= (a checkpoint of rvc/lib/predictors/FCPE.py's {'config', 'model'} "
                             "format, or its (state, config) pair); semantics='mlx' runs the MLX port's FCPE (its RMVPE "
                             "fallback)")

    def _fcpe(self, eng):
        """Load this pipeline's FCPE checkpoint into the engine (once per checkpoint). The handle is kept: while the
        engine still holds this checkpoint a call costs one comparison, not a hash of the state dict (fcpe_weights
        is read when it is first used; a state dict mutated in place afterwards is not noticed)."""
        m = getattr(self, "_fcpe_model", None)
        if m is not None and m.engine is eng and eng.loaded.get("fcpe") == m.key:
            return m
        src = self.fcpe_weights
        if isinstance(src, (tuple, list)):
            m = FCPE(eng, state=src[0], config=src[1])
        else:
            m = FCPE(eng, weights_path=src)
        self._fcpe_model = m
        return m

    def _crepe(self, eng, f0_method):
        """Load the CREPE weights f0_method names into the engine (once per model kind)."""
        kind = "tiny" if f0_method == "crepe-tiny" else "full"
        src = (self.crepe_weights or {}).get(kind)
        if isinstance(src, dict):
            return CREPE(kind, None, engine=eng, state=src)
        return CREPE(kind, src, engine=eng)

    def _f0_opts(self, eng, f0_method):
        """(f0_method, rmvpe_threshold) of rvcx_pipeline_opts for an f0 method name."""
        if f0_method in ("crepe", "crepe-tiny"):
            self._crepe(eng, f0_method)
            return (1 if self.semantics == "mlx" else 2), 0.03
        if f0_method == "fcpe":
            if self.semantics == "mlx":
                return 0, 0.006 * 5
            self._fcpe(eng)  # _check_method has made sure the weights were given
            return 3, 0.03
        return 0, 0.03

    @staticmethod
    def _check_guidance(eng, pitch_guidance: bool):
        """pitch_guidance must match the loaded model (infer.py:300 passes cpt["f0"]): the reference fails on a
        mismatch (pitchf.float() on None, pipeline.py:370; dec(z, None) for an NSF decoder); here it raises."""
        model_f0 = bool(eng.synth_cfg.use_f0)
        if pitch_guidance != model_f0:
            raise ValueError(f"pitch_guidance={pitch_guidance} but the loaded model has f0={int(model_f0)}")

    def _engine(self, *models):
        for mdl in models + (self.hubert_model, self.rmvpe_model):
            if mdl is not None and getattr(mdl, "engine", None) is not None:
                return mdl.engine
        if self.engine is None:
            raise RuntimeError("no rvcx Engine: pass models created by rvcx.infer (HubertModel/RMVPE0Predictor)")
        return self.engine

    def _ensure_highpass(self, eng):
        if getattr(eng, "_hp", None) is None:
            eng.set_pipeline_highpass(self.sample_rate)  # pipeline.py:22-27

    def set_tgt_sr(self, tgt_sr: int):
        """The output rate of the voice a call runs on (RVCX selects a voice per call): tgt_sr and the padding in
        output samples that follows from it."""
        self.tgt_sr = int(tgt_sr)
        self.t_pad_tgt = int(self.tgt_sr * self.x_pad)

    def load_index(self, file_index: str, eng=None):
        """faiss.read_index + reconstruct_n (pipeline.py:430-434) into the engine's current voice, cached per voice and
        (path, mtime, size): two voices that alternate each keep their own index resident."""
        from .index import IndexIVFFlat

        eng = eng or self._engine()
        st = os.stat(file_index)
        key = (os.path.abspath(file_index), st.st_mtime_ns, st.st_size, id(eng))
        cache = self.__dict__.setdefault("_index_cache", {})  # voice id -> (key, handle)
        hit = cache.get(eng.voice)
        if hit is None or hit[0] != key or eng.index_info() is None:
            cache[eng.voice] = hit = (key, IndexIVFFlat(eng, path=file_index))
        self._index_key, self.index = hit  # the last one asked for, as before
        return self.index

    # ------------------------------------------------------------------ API (pipeline_mlx.py:135-373)
    def get_f0(self, x, p_len, f0_method="rmvpe", pitch=0, f0_autotune=False, f0_autotune_strength=1.0,
               proposed_pitch=False, proposed_pitch_threshold=155.0):
        """-> (f0_coarse int64 [F], f0 float64 [F]) with F = 1 + len(x)//160 (pipeline.py:200-291)."""
        self._check_method(f0_method)
        eng = self._engine()
        method, thr = self._f0_opts(eng, f0_method)
        xa = np.asarray(x, dtype=np.float32).reshape(-1)
        if method == 1:  # PitchExtractor.extract -> CREPE.get_f0(x, f0_min=50, f0_max=1100) (pipeline_mlx.py:140)
            f0 = eng.crepe(xa, self.f0_min, self.f0_max, 0.1).double()
        elif method == 2:  # CREPE(...).get_f0(x, self.f0_min, self.f0_max, p_len, model) (pipeline.py:223-234)
            dither = None
            if self.crepe_dither:  # torchcrepe.convert.dither: scipy.stats.triang(c=0.5, loc=-20, scale=40)
                dither = np.random.default_rng().triangular(-20.0, 0.0, 20.0, size=1 + len(xa) // 160)
            f0 = eng.crepe(xa, self.f0_min, self.f0_max, 0.1, semantics="rvc", dither=dither).double()
        elif method == 3:  # FCPE(...).get_f0(x, p_len, filter_radius=0.006) (rvc/lib/predictors/f0.py:71-89)
            f0 = eng.fcpe(xa, self.fcpe_threshold)
        else:
            f0 = eng.rmvpe(xa, thr)
        shift = float(pitch)
        if f0_autotune:
            f0 = eng.f0_autotune(f0, f0_autotune_strength, skip_unvoiced=self.semantics == "mlx")
            if self.semantics == "rvc":
                shift = 0.0
        elif proposed_pitch and self.semantics == "rvc":
            shift += proposed_key(eng.host(f0), proposed_pitch_threshold)
        coarse, _, fs = eng.f0_post(f0, shift)
        return eng.host(coarse).astype(np.int64), eng.host(fs)

    def voice_conversion(self, model, net_g, sid, audio0, pitch, pitchf, index=None, big_npy=None, index_rate=0.0,
                         version="v2", protect=0.33, eps_z=None, eps_src=None, seed: int = 0):
        """One padded chunk: HuBERT -> x2 -> protect -> Synthesizer.infer. -> float32 [p_len * upp].
        pitch / pitchf None = pitch_guidance False (pipeline.py:324): no protect, the model's f0-less decoder."""
        eng = self._engine(model)
        self._check_guidance(eng, pitch is not None and pitchf is not None)
        rate = 0.0
        if index is not None and index_rate > 0:  # pipeline.py:338-342 (big_npy is the index's own rows)
            if getattr(index, "engine", None) is not eng:
                raise TypeError("index must be an rvcx IndexIVFFlat loaded on this pipeline's engine (read_index)")
            index._bound()
            rate = float(index_rate)
        out = eng.voice_conversion(np.asarray(audio0, dtype=np.float32).reshape(-1),
                                   None if pitch is None else _np(pitch).reshape(-1),
                                   None if pitchf is None else _np(pitchf).reshape(-1), int(_np(sid).reshape(-1)[0]),
                                   float(protect),
                                   eps_z=eps_z, eps_src=eps_src, seed=seed, index_rate=rate)
        return eng.host(out)

    def pipeline(self, model, net_g, sid, audio, pitch=0, f0_method="rmvpe", file_index=None, index_rate=0.0,
                 pitch_guidance=True, volume_envelope=1.0, version="v2", protect=0.33, f0_autotune=False,
                 f0_autotune_strength=1.0, proposed_pitch=False, proposed_pitch_threshold=155.0, eps_z=None,
                 eps_src=None, seed: int = 0, post=None):
        """Whole utterance -> float32 [N_out] @tgt_sr (pipeline.py:390-558). audio: a numpy array or a device tensor
        (as the device loader returns it). post (device tensor -> device tensor) runs on the output before its copy
        to the host (the resample_sr stage of rvcx.infer.RVCX)."""
        eng, opts = self._pipeline_opts(model, sid, pitch, f0_method, file_index, index_rate, pitch_guidance,
                                        volume_envelope, version, protect, f0_autotune, f0_autotune_strength,
                                        proposed_pitch, proposed_pitch_threshold)
        y, f0 = eng.pipeline_ex(_row(audio), opts, eps_z=eps_z, eps_src=eps_src, seed=seed, want_f0=True)
        self.last_f0 = f0
        return eng.host(y if post is None else post(y))

    def _pipeline_opts(self, model, sid, pitch, f0_method, file_index, index_rate, pitch_guidance, volume_envelope,
                       version, protect, f0_autotune, f0_autotune_strength, proposed_pitch, proposed_pitch_threshold):
        """The checks and the rvcx_pipeline_opts of one `pipeline` call -> (engine, opts)."""
        self._check_method(f0_method)
        eng = self._engine(model)
        self._check_guidance(eng, bool(pitch_guidance))
        # pipeline.py:430-436: the index is used only when the file exists and index_rate > 0 (a missing
        # file means no retrieval, as in the reference); a file that does not parse raises here.
        rate = 0.0
        if file_index and os.path.exists(file_index) and index_rate > 0:
            self.load_index(file_index, eng)
            rate = float(index_rate)
        self._ensure_highpass(eng)
        method, thr = self._f0_opts(eng, f0_method)
        mlx = self.semantics == "mlx"
        t_pad = 1600 if mlx else self.t_pad
        t_pad_tgt = int(t_pad * self.tgt_sr / self.sample_rate) if mlx else self.t_pad_tgt
        opts = eng.pipeline_opts(
            sid=int(_np(sid).reshape(-1)[0]), version={"v1": 1, "v2": 2}.get(version, 0), pitch=float(pitch),
            protect=float(protect), t_pad=t_pad, t_pad_tgt=t_pad_tgt, t_query=self.t_query,
            t_center=self.t_center, t_max=0 if mlx else self.t_max, f0_autotune=int(bool(f0_autotune)),
            f0_autotune_strength=float(f0_autotune_strength),
            proposed_pitch=int(bool(proposed_pitch) and not mlx),
            proposed_pitch_threshold=float(proposed_pitch_threshold), volume_envelope=float(volume_envelope),
            mlx_semantics=int(mlx), index_rate=rate, f0_method=method, rmvpe_threshold=thr,
            fcpe_threshold=self.fcpe_threshold)
        return eng, opts

    def pipeline_many(self, model, net_g, sid, audios, pitch=0, f0_method="rmvpe", file_index=None, index_rate=0.0,
                      pitch_guidance=True, volume_envelope=1.0, version="v2", protect=0.33, f0_autotune=False,
                      f0_autotune_strength=1.0, proposed_pitch=False, proposed_pitch_threshold=155.0, seed: int = 0,
                      batch: int = DEFAULT_BATCH, max_pad: float = DEFAULT_MAX_PAD, noise_fn=None,
                      ragged_f0: bool = False, post=None, voices=None):
        """`pipeline` over a list of utterances of any lengths -> the list of float32 outputs in input order.
        voices: None (every utterance on the engine's current voice), or one ``VoiceRef`` per utterance, in any order
        (the voices of rvcx.infer.RVCX): the utterances are first split by what the voices of one batch must share
        (the synthesizer's geometry, and whether the voice retrieves), then bucketed by length as below; each batch's
        rows are ordered by voice and go through one rvcx_pipeline_batch_voices pass -- HuBERT and the pitch network
        once over all rows, retrieval and the synthesizer once per voice. pitch_guidance, version and file_index are
        then each voice's own (file_index here is the fallback for a voice without one); `post` must serve every voice.
        The utterances are grouped longest first into batches of up to `batch` rows whose shortest is at least
        (1 - max_pad) of the longest (rvcx.offline.bucket) and every batch is one rvcx_pipeline_batch_v pass; an
        utterance above t_max goes through `pipeline` alone (the batched pass takes single-chunk rows). batch = 1 is
        the per-utterance loop. Batch k draws its noise from seed + k; noise_fn(i, T) -> (eps_z [inter, T], eps_src
        [T * upp]) injects utterance i's noise instead (T its synthesizer frames), as the tests do.
        ragged_f0 (f0_method "rmvpe" or "fcpe", else ValueError): the rows of a batch share one ragged pass of the pitch
        network (rvcx_pipeline_opts.f0_method 4 for RMVPE, 5 for the FCPE network) instead of one pass per row; a row's
        f0 then equals the per-row pass up to summation order, not bit for bit.
        An utterance may be a device tensor (the device loader's rows): it stays on the device. post (device tensor ->
        device tensor) runs on every output before its copy to the host."""
        from ..offline import bucket

        if ragged_f0 and f0_method not in ("rmvpe", "fcpe"):
            raise ValueError(f'ragged_f0 runs RMVPE or FCPE: f0_method must be "rmvpe" or "fcpe", not {f0_method!r}')
        if voices is not None:
            return self._pipeline_many_voices(
                model, sid, audios, voices, pitch, f0_method, file_index, index_rate, volume_envelope, protect,
                f0_autotune, f0_autotune_strength, proposed_pitch, proposed_pitch_threshold, seed, batch, max_pad,
                noise_fn, ragged_f0, post)

        eng, opts = self._pipeline_opts(model, sid, pitch, f0_method, file_index, index_rate, pitch_guidance,
                                        volume_envelope, version, protect, f0_autotune, f0_autotune_strength,
                                        proposed_pitch, proposed_pitch_threshold)
        if ragged_f0:  # "fcpe" is method 3 with its network loaded, method 0 as the MLX port's RMVPE fallback
            opts.f0_method = 5 if int(opts.f0_method) == 3 else 4
        audios = [_row(a) for a in audios]
        outs = [None] * len(audios)
        upp = eng.upp

        def host(y):
            return eng.host(y if post is None else post(y))

        def noise(i):
            return (None, None) if noise_fn is None else noise_fn(i, eng.pipeline_frames(len(audios[i]), opts))

        t_max = int(opts.t_max)
        short = [i for i, a in enumerate(audios) if not (t_max > 0 and len(a) + 160 > t_max)]
        for i in sorted(set(range(len(audios))) - set(short)):  # long inputs: the split search and the chunk loop
            outs[i] = host(eng.pipeline_ex(audios[i], opts, seed=seed))
        for k, g in enumerate(bucket([len(audios[i]) for i in short], max(1, int(batch)), float(max_pad))):
            ids = [short[j] for j in g]
            if len(ids) == 1:
                ez, es = noise(ids[0])
                outs[ids[0]] = host(eng.pipeline_ex(audios[ids[0]], opts, eps_z=ez, eps_src=es, seed=seed + k))
                continue
            ez = es = None
            if noise_fn is not None:
                Ts = [eng.pipeline_frames(len(audios[i]), opts) for i in ids]
                per = [noise(i) for i in ids]
                ez = np.zeros((len(ids), per[0][0].shape[0], max(Ts)), np.float32)
                es = np.zeros((len(ids), max(Ts) * upp), np.float32)
                for r, (z, sct) in enumerate(per):
                    ez[r, :, :Ts[r]] = z
                    es[r, :Ts[r] * upp] = sct
            ys = eng.pipeline_batch_v([audios[i] for i in ids], opts, sids=int(opts.sid), eps_z=ez, eps_src=es,
                                      seed=seed + k)
            eng.check_device_status()
            for i, y in zip(ids, ys):
                outs[i] = (y if post is None else post(y)).cpu().numpy()
        return outs

    def _pipeline_many_voices(self, model, sid, audios, voices, pitch, f0_method, file_index, index_rate,
                              volume_envelope, protect, f0_autotune, f0_autotune_strength, proposed_pitch,
                              proposed_pitch_threshold, seed, batch, max_pad, noise_fn, ragged_f0, post):
        """pipeline_many with a VoiceRef per utterance. post: None, or {voice id: device tensor -> device tensor}."""
        from ..offline import bucket_voices

        eng = self._engine(model)
        audios = [_row(a) for a in audios]
        voices = list(voices)
        if len(voices) != len(audios):
            raise ValueError(f"voices has {len(voices)} entries for {len(audios)} utterances")
        back, back_sr = eng.voice, self.tgt_sr
        post = post or {}
        try:
            # per voice: its checks, its index (loaded into that voice) and its options; what its batch must share
            by_id, opts, keys = {}, {}, {}
            for v in voices:
                if v.id in by_id:
                    continue
                by_id[v.id] = v
                eng.select_voice(v.id)
                self.set_tgt_sr(v.tgt_sr)
                _, o = self._pipeline_opts(model, sid, pitch, f0_method, v.file_index or file_index, index_rate,
                                           v.pitch_guidance, volume_envelope, v.version, protect, f0_autotune,
                                           f0_autotune_strength, proposed_pitch, proposed_pitch_threshold)
                if ragged_f0:
                    o.f0_method = 5 if int(o.f0_method) == 3 else 4
                opts[v.id] = o
                keys[v.id] = voice_key(eng.synth_cfg, o.index_rate > 0)
            vids = [v.id for v in voices]
            outs = [None] * len(audios)

            def host(y, vid):
                return eng.host(y if post.get(vid) is None else post[vid](y))

            def noise(i):
                if noise_fn is None:
                    return None, None
                return noise_fn(i, eng.pipeline_frames(len(audios[i]), opts[vids[i]]))

            def alone(i, **kw):
                eng.select_voice(vids[i])
                return host(eng.pipeline_ex(audios[i], opts[vids[i]], **kw), vids[i])

            t_max = int(next(iter(opts.values())).t_max)
            short = [i for i, a in enumerate(audios) if not (t_max > 0 and len(a) + 160 > t_max)]
            for i in sorted(set(range(len(audios))) - set(short)):
                outs[i] = alone(i, seed=seed)
            plan = bucket_voices([len(audios[i]) for i in short], [vids[i] for i in short], keys, max(1, int(batch)),
                                 float(max_pad))
            for k, g in enumerate(plan):
                ids = [short[j] for j in g]
                if len(ids) == 1:
                    ez, es = noise(ids[0])
                    outs[ids[0]] = alone(ids[0], eps_z=ez, eps_src=es, seed=seed + k)
                    continue
                o = opts[vids[ids[0]]]
                ez = es = None
                if noise_fn is not None:
                    upp = eng.voice_info(vids[ids[0]])["upp"]
                    Ts = [eng.pipeline_frames(len(audios[i]), o) for i in ids]
                    per = [noise(i) for i in ids]
                    ez = np.zeros((len(ids), per[0][0].shape[0], max(Ts)), np.float32)
                    es = np.zeros((len(ids), max(Ts) * upp), np.float32)
                    for r, (z, sct) in enumerate(per):
                        ez[r, :, :Ts[r]] = z
                        es[r, :Ts[r] * upp] = sct
                ys = eng.pipeline_batch_v([audios[i] for i in ids], o, sids=int(o.sid), eps_z=ez, eps_src=es,
                                          seed=seed + k, voices=[vids[i] for i in ids])
                eng.check_device_status()
                for i, y in zip(ids, ys):
                    outs[i] = (y if post.get(vids[i]) is None else post[vids[i]](y)).cpu().numpy()
            return outs
        finally:
            eng.select_voice(back)
            self.set_tgt_sr(back_sr)


PipelineMLX = PipelineRVCX


def _row(audio):
    """One utterance as the engine takes it: fp64 [n], a torch tensor passed through, anything else as numpy."""
    if hasattr(audio, "data_ptr"):
        return audio.double().reshape(-1)
    return np.asarray(audio, dtype=np.float64).reshape(-1)


def proposed_key(f0: np.ndarray, threshold: float, limit: int = 12) -> int:
    """Key offset of proposed_pitch (rvc/infer/pipeline.py:250-277)."""
    valid = np.where(f0 > 0)[0]
    if len(valid) < 2:
        return 0
    med = float(np.median(np.interp(np.arange(len(f0)), valid, f0[valid])))
    if med <= 0 or np.isnan(med):
        return 0
    return max(-limit, min(limit, int(np.round(12 * np.log2(threshold / med)))))
